// gpu_batch_internal.h -- declarations shared by the translation units of class GpuBatch (gpu_batch.cpp: lifecycle and launch
// dispatch; gpu_batch_chains.cpp: half-batch chains, resident launch, timing marks; gpu_batch_host.cpp: host-buffer entry points; gpu_batch_snapshot.cpp: stream snapshots).
// Which route a processing call takes is not decided here but in host_route.h (host data only); what the next launch has to come
// behind is InFlight below, the one member of GpuBatch that says what is in flight where.
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

	// What of this batch is in flight where, as far as the NEXT launch has to know: the stream state makes every kernel launch depend on
	// the one before it, whichever stream either runs on (batch stream, a slot's own stream, the chain streams).  The resident launch
	// keeps its own books (ResidentState).
	struct GpuBatch::InFlight
	{
		// a buffer has gone through Submit on a slot stream or the chains, so work of this batch may sit on streams other than the batch
		// stream.  Never cleared.  Every assignment of `lastKernelEvent` sets it first, so `lastKernelEvent != nullptr` implies it: the
		// sites that asked for `pipelineUsed && lastKernelEvent` asked for `lastKernelEvent`.
		bool pipelineUsed = false;
		// the event behind the last kernel launched outside the free-running forms, and the stream it was recorded on; both null: none,
		// or the last kernels ran on the chains (whoever comes next drains those itself: JoinHalves, BeginHalves)
		hipEvent_t lastKernelEvent = nullptr;
		hipStream_t lastKernelStream = nullptr;
		// the last Submit ran its kernel on the batch stream (pinned blocks read in place), with no event behind it: the next buffer on a
		// slot stream waits for the batch stream first
		bool lastSubmitOnBatchStream = false;
		// the topology version whose state resets and index lists the slot streams / the chains have been put behind
		unsigned long submitTopology = 0;
		// the chain streams may hold work of this batch; cleared by whoever has waited for all of them (WaitChains)
		bool halfChainsUsed = false;
		// recorded on the batch stream for a stream that has to come behind it; created on first use (or by EnsureMainDone on the set-up side)
		hipEvent_t mainDone = nullptr;

		// `s` comes behind the last kernel (nothing to do when that ran on `s` itself)
		void OrderBehindLastKernel(hipStream_t s) const
		{
			if (lastKernelEvent && lastKernelStream != s) CheckHip(hipStreamWaitEvent(s, lastKernelEvent, 0), "hipStreamWaitEvent");
		}
		void NoteLastKernel(hipEvent_t event, hipStream_t s)
		{
			pipelineUsed = true;
			lastKernelEvent = event;
			lastKernelStream = s;
		}
		void NoteNoLastKernel() { NoteLastKernel(nullptr, nullptr); }
		void EnsureMainDone()
		{
			if (!mainDone) CheckHip(CountedHipEventCreateWithFlags(&mainDone, hipEventDisableTiming), "hipEventCreate");
		}
		hipEvent_t RecordMainDone(hipStream_t batchStream)
		{
			EnsureMainDone();
			CheckHip(hipEventRecord(mainDone, batchStream), "hipEventRecord");
			return mainDone;
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

	// The ring of entry tables of a per-stream stage: pinned and device blocks of `capacity` entries and an event each.  One table more
	// than buffers can be in flight (Submit): the table a call takes was read by a launch whose ticket has been collected.  `name` is
	// the stage's in the messages.  A processing call steps through Take, the book's BuildTable, Upload, its launches and Commit.
	template <class Entry>
	struct StageTables
	{
		static constexpr int kTables = GpuBatch::kPipelineSlots + 1;
		const std::string name, inFlight, uploadWhat;
		Entry* host[kTables] = {};     // pinned
		Entry* dev[kTables] = {};
		hipEvent_t done[kTables] = {}; // the launches that read dev[i] (and the upload that read host[i]) are over
		bool used[kTables] = {};
		int next = 0;
		int capacity = 0;              // entries per table
		explicit StageTables(const char* stage) : name(stage), inFlight(name + ": table in flight"), uploadWhat("hipMemcpyAsync (" + name + " table)") {}
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
				if (used[i]) batch.WaitEventBounded(done[i], inFlight.c_str());
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
		// the call does not fit what the set-up side sized (`fits` false): a table with more than `capacity` entries, a row past the stage's blocks
		void Require(bool fits) const
		{
			if (!fits) throw std::runtime_error("neuralaudio_amd: " + name + ": more entries than the tables hold");
		}
		// the next table for a call of up to `entries` entries, pinned block and device twin, once the launch that last read it is over (a
		// bounded wait)
		struct Table
		{
			Entry *host, *dev;
		};
		Table Take(GpuBatch& batch, int entries)
		{
			Require(entries <= capacity);
			if (used[next]) batch.WaitEventBounded(done[next], inFlight.c_str());
			return { host[next], dev[next] };
		}
		// the first `units` entries of the table taken go to its device twin, in front of the launches that read it
		void Upload(const Table& table, int units, hipStream_t stream) const
		{
			CheckHip(hipMemcpyAsync(table.dev, table.host, (size_t)units * sizeof(Entry), hipMemcpyHostToDevice, stream), uploadWhat.c_str());
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

	// The result blocks of a stage that reports to the host (meter, tuner) -- the one device -> host path of the stages.  A block per table
	// of the stage's ring: a launch of the call that took table i writes records to dev[i], one copy brings them to the pinned host[i],
	// the table's `done` event covers the copy, and the host folds what has arrived into the book without ever waiting for it.
	template <class Record>
	struct GpuBatch::StageResults
	{
		static constexpr int kTables = GpuBatch::kPipelineSlots + 1;
		Record* host[kTables] = {}; // pinned: the records of the call that last used table i ...
		Record* dev[kTables] = {};  // ... and where its launch wrote them
		int pending[kTables] = {};  // records of host[i] that have not been folded yet (0: none)
		int capacity = 0;           // records per block
		~StageResults() { Free(); }
		// set-up side: blocks of at least `want` records.  Records that have not arrived are given up with their blocks: whatever writes
		// them is over first, and the entries they belong to report again with their next window
		void Ensure(GpuBatch& batch, int want)
		{
			if (want <= capacity) return;
			if (capacity > 0) batch.Quiesce();
			Free();
			for (int i = 0; i < kTables; i++)
			{
				CheckHip(CountedHipHostMalloc(reinterpret_cast<void**>(&host[i]), (size_t)want * sizeof(Record), hipHostMallocDefault), "hipHostMalloc");
				CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dev[i]), (size_t)want * sizeof(Record)), "hipMalloc");
			}
			capacity = want;
		}
		// the first `count` records of dev[i] come to host[i], behind the launch that wrote them and in front of table i's Commit
		void Download(int i, int count, hipStream_t stream, const char* what)
		{
			CheckHip(hipMemcpyAsync(host[i], dev[i], (size_t)count * sizeof(Record), hipMemcpyDeviceToHost, stream), what);
			pending[i] = count;
		}
		// the pending records of block i go through the stage's `fold(i, count)`; Take of table i folds before the block is written again
		template <class Fold>
		void FoldBlock(int i, Fold&& fold)
		{
			if (pending[i]) fold(i, pending[i]);
			pending[i] = 0;
		}
		// Event queries only: every block whose copy is over is folded.  The blocks complete in the order of their calls (every call's
		// launches come behind the call before), so the walk starts at the oldest and ends at the first that is not over.
		template <class Entry, class Fold>
		void Poll(const StageTables<Entry>& tables, const char* what, Fold&& fold)
		{
			for (int k = 0; k < kTables; k++)
			{
				const int i = (tables.next + k) % kTables;
				if (pending[i] == 0) continue;
				const hipError_t q = hipEventQuery(tables.done[i]);
				if (q == hipErrorNotReady)
				{
					(void)hipGetLastError(); // (not an error of anything that follows)
					return;
				}
				CheckHip(q, what);
				FoldBlock(i, fold);
			}
		}
		long long Bytes() const { return (long long)kTables * capacity * (long long)sizeof(Record); }

	private:
		void Free()
		{
			capacity = 0;
			for (int i = 0; i < kTables; i++)
			{
				pending[i] = 0;
				if (host[i]) (void)CountedHipHostFree(host[i]);
				if (dev[i]) (void)CountedHipFree(dev[i]);
				host[i] = dev[i] = nullptr;
			}
		}
	};

	// the argument checks the stages' calls share: the texts are part of the interface (the tests match on them)
	inline std::string StreamId(int s) { return "stream " + std::to_string(s); }
	inline void RequireFadeRange(int samples, const char* who, const char* argument)
	{
		if (samples < 0 || samples > kOutStageMaxRamp) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": " + argument + " must lie in [0, 1 << 20]");
	}

	// What the eleven stages share (GpuBatch::Stage, gpu_batch.h): the host mirror `book` (its own header, host-compilable) and the ring of
	// entry tables.
	template <class Book, class Entry>
	struct GpuBatch::StageOf : GpuBatch::Stage
	{
		Book book;
		StageTables<Entry> tables;
		explicit StageOf(const char* name) : tables(name) {}
		bool HasEntries() const override { return book.HasEntries(); }
	};

	// the gate stage (gate_stage.h, gate_stage.cpp): the rows' states and gain rows on the device, and -- between the
	// detector and the apply launch of one call -- the table that call runs on
	struct GpuBatch::GateStage : StageOf<GateBook, GateEntry>
	{
		static constexpr StageId kId = kGateStage;
		static constexpr const char* kNotEnabled = "gate stage not enabled (NA_BatchEnableGateStage)";
		float* state = nullptr;           // [rowCapacity] GateState
		float* gains = nullptr;           // [rowCapacity][gainSamples]
		int rowCapacity = 0;
		int gainSamples = kGateMinGainSamples; // a power of two
		const GateEntry* dev = nullptr;   // the device table the detector of this call read ...
		int count = 0;                    // ... and its entries; 0: the call has none
		GateStage() : StageOf("gate stage") {}
		~GateStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // its gate goes at once
		void EnsureSamples(GpuBatch& batch, size_t n); // gain rows of at least n samples (grows them: not real-time safe)
		void BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride) override; // table upload + the detector launch
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override;              // the apply launch + the host mirror's advance
	};
	hipError_t LaunchGateDetect(const GateDetectLaunch& L, hipStream_t stream); // (gate_stage_kernels.hip)
	hipError_t LaunchGateApply(const GateApplyLaunch& L, hipStream_t stream);

	// the EQ stage (eq_stage.h, eq_stage.cpp): the rows' two slots of coefficients and section states on the device; its
	// tables hold the entries and behind them the coefficient sets of the set calls since the last call
	struct GpuBatch::EqStage : StageOf<EqBook, EqEntry>
	{
		static constexpr StageId kId = kEqStage;
		static constexpr const char* kNotEnabled = "eq stage not enabled (NA_BatchEnableEqStage)";
		float* coefs = nullptr;           // [rowCapacity][2] EqCoefSet
		float* state = nullptr;           // [rowCapacity][2][kEqMaxSections] EqSecState
		int rowCapacity = 0;
		EqStage() : StageOf("eq stage") {}
		~EqStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // flat at once, its states dropped
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override; // table upload + launch + the host mirror's advance
	};
	hipError_t LaunchEqStage(const EqLaunch& L, hipStream_t stream); // (eq_stage_kernels.hip)

	// the cabinet stage (cabinet_stage.h, cabinet_stage.cpp): the rows' history rings and the IRs' taps (owned through
	// the book's ids)
	struct GpuBatch::CabinetStage : StageOf<CabinetBook, CabEntry>
	{
		static constexpr StageId kId = kCabinetStage;
		static constexpr const char* kNotEnabled = "cabinet stage not enabled (NA_BatchEnableCabinetStage)";
		float* rings = nullptr;           // [ringRows][book.RingSamples()]
		int ringRows = 0;
		long long tapBytes = 0;           // device bytes of the loaded IRs
		CabinetStage() : StageOf("cabinet stage") {}
		~CabinetStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // dry at once, its history dropped
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override; // table upload + two launches per piece + the host mirror's advance
	};
	hipError_t LaunchCabinetStage(const CabLaunch& L, hipStream_t stream); // (cabinet_stage_kernels.hip) the two launches of one piece

	// the compressor stage (compressor_stage.h, compressor_stage.cpp): the rows' two curve slots and states on the
	// device; its tables hold the entries and behind them the curves of the set calls since the last call
	struct GpuBatch::CompressorStage : StageOf<CompBook, CompEntry>
	{
		static constexpr StageId kId = kCompressorStage;
		static constexpr const char* kNotEnabled = "compressor stage not enabled (NA_BatchEnableCompressorStage)";
		float* curves = nullptr;          // [rowCapacity][2] CompCurve
		float* state = nullptr;           // [rowCapacity] CompState
		int rowCapacity = 0;
		CompressorStage() : StageOf("compressor stage") {}
		~CompressorStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // no compressor at once, its state dropped
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override; // table upload + launch + the host mirror's advance
	};
	hipError_t LaunchCompressorStage(const CompLaunch& L, hipStream_t stream); // (compressor_stage_kernels.hip)

	// the modulation stage (mod_stage.h, mod_stage.cpp): the rows' lines (rings)
	struct GpuBatch::ModStage : StageOf<ModBook, ModEntry>
	{
		static constexpr StageId kId = kModStage;
		static constexpr const char* kNotEnabled = "modulation stage not enabled (NA_BatchEnableModStage)";
		float* rings = nullptr;           // [ringRows][book.RingSamples()]
		int ringRows = 0;
		ModStage() : StageOf("modulation stage") {}
		~ModStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // no modulation at once, its history dropped
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override; // table upload + one launch per piece + the host mirror's advance
	};
	hipError_t LaunchModStage(const ModLaunch& L, hipStream_t stream); // (mod_stage_kernels.hip) the launch of one piece

	// the delay stage (delay_stage.h, delay_stage.cpp): the rows' delay lines (rings) and filter states
	struct GpuBatch::DelayStage : StageOf<DelayBook, DelayEntry>
	{
		static constexpr StageId kId = kDelayStage;
		static constexpr const char* kNotEnabled = "delay stage not enabled (NA_BatchEnableDelayStage)";
		float* rings = nullptr;           // [ringRows][book.RingSamples()]
		float* state = nullptr;           // [stateRows] DelayFilter
		int ringRows = 0, stateRows = 0;
		DelayStage() : StageOf("delay stage") {}
		~DelayStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // no delay at once, its history dropped
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override; // table upload + one launch per piece + the host mirror's advance
	};
	hipError_t LaunchDelayStage(const DelayLaunch& L, hipStream_t stream); // (delay_stage_kernels.hip) the launch of one piece

	// the reverb stage (reverb_stage.h, reverb_stage.cpp): the rows' sample rings, rings of input spectra and tail blocks,
	// the transform's twiddles and the IRs' head taps and partition spectra (owned through the book's ids)
	struct GpuBatch::ReverbStage : StageOf<ReverbBook, RevEntry>
	{
		static constexpr StageId kId = kReverbStage;
		static constexpr const char* kNotEnabled = "reverb stage not enabled (NA_BatchEnableReverbStage)";
		float* rings = nullptr;           // [ringRows][kRevRingSamples]
		float* tails = nullptr;           // [ringRows][kRevTailFloats]
		float* spectra = nullptr;         // [spectraRows][book.Slots()][kRevSpectrumFloats]
		float* twiddles = nullptr;        // [kRevPoints]
		int ringRows = 0, spectraRows = 0;
		long long irBytes = 0;            // device bytes of the loaded IRs
		ReverbStage() : StageOf("reverb stage") {}
		~ReverbStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // no reverb at once, its history dropped
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override; // table upload + up to four launches per piece + the host mirror's advance
	};
	hipError_t LaunchReverbStage(const RevLaunch& L, hipStream_t stream); // (reverb_stage_kernels.hip) the launches of one piece
	hipError_t LaunchReverbIR(const RevIRLaunch& L, hipStream_t stream);  // ... and of one IR's spectra, load side

	// the output stage (output_stage.h, output_stage.cpp)
	struct GpuBatch::OutputStage : StageOf<OutputStageBook, OutStageEntry>
	{
		static constexpr StageId kId = kOutputStage;
		static constexpr const char* kNotEnabled = "output stage not enabled (NA_BatchEnableOutputStage)";
		OutputStage() : StageOf("output stage") {}
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override; // its fade ends, its gain is 1 again
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override; // table upload + launch + the host mirror's advance
	};
	hipError_t LaunchOutputStage(const OutStageLaunch& L, hipStream_t stream); // (output_stage_kernels.hip)

	// the mix stage (mix_stage.h, mix_stage.cpp): the groups' matrices and the stashed input rows of DRY members on the
	// device; its tables hold the entries and behind them the gain sets of the set calls since the last call, and -- between the stash
	// launch and the mix launch of one call -- the table that call runs on
	struct GpuBatch::MixStage : StageOf<MixBook, MixEntry>
	{
		static constexpr StageId kId = kMixStage;
		static constexpr const char* kNotEnabled = "mix stage not enabled (NA_BatchEnableMixStage)";
		float* gains = nullptr;           // [rowCapacity][2][8][8]: a group's from / to matrices, at the row of its first member
		float* stash = nullptr;           // [rowCapacity][drySamples]: the input rows of DRY members (nothing of it outlives its call)
		int rowCapacity = 0;
		int drySamples = kMixMinDrySamples; // a power of two
		const MixEntry* dev = nullptr;    // the device table this call runs on ...
		int count = 0;                    // ... and its entries; 0: the call has none
		MixStage() : StageOf("mix stage") {}
		~MixStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // the group that names it goes at once
		void EnsureSamples(GpuBatch& batch, size_t n); // stash rows of at least n samples (grows them: not real-time safe)
		void BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride) override; // table upload (+ the stash launch)
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override;              // the mix launch + the host mirror's advance
	};
	hipError_t LaunchMixStash(const MixStashLaunch& L, hipStream_t stream); // (mix_stage_kernels.hip)
	hipError_t LaunchMixStage(const MixLaunch& L, hipStream_t stream);

	// the meter stage (meter_stage.h, meter_stage.cpp): the rows' states on the device and the result blocks (StageResults
	// above) the OUT launch writes a record per entry to
	struct GpuBatch::MeterStage : StageOf<MeterBook, MeterEntry>
	{
		static constexpr StageId kId = kMeterStage;
		static constexpr const char* kNotEnabled = "meter stage not enabled (NA_BatchEnableMeterStage)";
		float* state = nullptr;             // [rowCapacity] MeterState
		int rowCapacity = 0;
		StageResults<MeterRecord> results;
		const MeterEntry* dev = nullptr;    // the device table the IN launch of this call read ...
		int count = 0;                      // ... and its entries; 0: the call has none
		int slot = 0;                       // ... and its place in the ring
		bool anyGated = false;              // ... and whether one of them is an entry of the gate stage in this call
		MeterStage() : StageOf("meter stage") {}
		~MeterStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // its meter goes at once
		void Fold(int i, int records); // the records of results.host[i] go into the book (stale ones are dropped there)
		void Poll() { results.Poll(tables, "hipEventQuery (meter results)", [this](int i, int records) { Fold(i, records); }); }
		void BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride) override; // poll + table upload + the IN launch
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override;              // the OUT launch + the result copy + the host mirror's advance
	};
	hipError_t LaunchMeterIn(const MeterLaunch& L, hipStream_t stream); // (meter_stage_kernels.hip)
	hipError_t LaunchMeterOut(const MeterLaunch& L, hipStream_t stream);

	// the tuner stage (tuner_stage.h, tuner_stage.cpp): the rows' open groups and rings of decimated samples on the
	// device and a result block per table of the ring, read back the way the meter stage's are; everything a call enqueues is in
	// BeforeModels (the rows it reads may be the rows the models write)
	struct GpuBatch::TunerStage : StageOf<TunerBook, TunerEntry>
	{
		static constexpr StageId kId = kTunerStage;
		static constexpr const char* kNotEnabled = "tuner stage not enabled (NA_BatchEnableTunerStage)";
		float* state = nullptr;             // [rowCapacity] TunerState
		float* rings = nullptr;             // [rowCapacity][kTunerRingSamples] int32
		int rowCapacity = 0;
		StageResults<TunerRecord> results;  // the evaluate launch writes a record per evaluating entry
		TunerStage() : StageOf("tuner stage") {}
		~TunerStage() override;
		void EnsureRows(GpuBatch& batch, int rows) override;
		void Leave(int s) override { if (s < book.Rows()) book.Leave(s); } // its tuner goes at once
		void Fold(int i, int records); // the records of results.host[i] go into the book (stale ones are dropped there)
		void Poll() { results.Poll(tables, "hipEventQuery (tuner results)", [this](int i, int records) { Fold(i, records); }); }
		void BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride) override; // poll + table upload + append (+ evaluate + result copy) + the host mirror's advance
		void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) override;              // nothing
	};
	hipError_t LaunchTunerAppend(const TunerLaunch& L, hipStream_t stream); // (tuner_stage_kernels.hip)
	hipError_t LaunchTunerEvaluate(const TunerLaunch& L, hipStream_t stream);

	// the stage S of the batch; throws "<who>: <stage> not enabled (...)" -- the text is part of the interface
	template <class S>
	S& GpuBatch::Require(const char* who) const
	{
		Stage* stage = stages[S::kId].get();
		if (!stage) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": " + S::kNotEnabled);
		return static_cast<S&>(*stage);
	}

	// set-up side of every NA_BatchEnable*Stage: the stage, with what the rows the batch has need on the device
	template <class S>
	S& GpuBatch::EnableStage()
	{
		CheckUsable();
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!stages[S::kId]) stages[S::kId].reset(new S());
		stages[S::kId]->EnsureRows(*this, (int)streams.size());
		EnsurePoolPipeline(); // (an entry moves Submit's buffers onto the slots' own streams or the copy streams: they exist from here on)
		return static_cast<S&>(*stages[S::kId]);
	}

	// the preamble of a set call on a stream: a usable batch, the stage, a stream that is live and not parked
	template <class S>
	S& GpuBatch::SettableStage(int s, const char* who)
	{
		CheckUsable();
		S& stage = Require<S>(who);
		if (IsParked(s)) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": " + StreamId(s) + " is parked");
		if (!IsLive(s)) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": " + StreamId(s) + " is not a live stream of the batch");
		return stage;
	}

	bool HostDirect(); // (gpu_batch_host.cpp) the kernels read / write pinned host blocks themselves instead of the copy engines
}
