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
		bool inside = false;        // the model launches of a resampled call are under way (ProcessDeviceOn)
		int lastFrames = 0, lastRows = 0; // NA_DebugResampleTap: model frames and rows of the last piece
		~ResampleState()
		{
			for (float* p : { tableUp, tableDown, histUp, histDown, modelIn, modelOut })
				if (p) (void)CountedHipFree(p);
		}
	};

	// the output stage of a batch (output_stage.h): the host mirror and the ring of entry tables
	struct GpuBatch::OutputStage
	{
		// one table more than buffers can be in flight (Submit): the table a call takes was read by a launch whose ticket has been collected
		static constexpr int kTables = GpuBatch::kPipelineSlots + 1;
		OutputStageBook book;
		OutStageEntry* host[kTables] = {}; // pinned
		OutStageEntry* dev[kTables] = {};
		hipEvent_t done[kTables] = {};     // the launch that read dev[i] (and the upload that read host[i]) is over
		bool used[kTables] = {};
		int next = 0;
		int capacity = 0;             // entries per table
		~OutputStage()
		{
			for (int i = 0; i < kTables; i++)
			{
				if (host[i]) (void)CountedHipHostFree(host[i]);
				if (dev[i]) (void)CountedHipFree(dev[i]);
				if (done[i]) (void)hipEventDestroy(done[i]);
			}
		}
	};
	hipError_t LaunchOutputStage(const OutStageLaunch& L, hipStream_t stream); // (output_stage_kernels.hip)

	// the cabinet stage of a batch (cabinet_stage.h): the host mirror, the rows' history rings, the IRs' taps (owned
	// through the book's ids) and the ring of entry tables
	struct GpuBatch::CabinetStage
	{
		static constexpr int kTables = GpuBatch::kPipelineSlots + 1; // (as the output stage's)
		CabinetBook book;
		float* rings = nullptr;           // [ringRows][book.RingSamples()]
		int ringRows = 0;
		long long tapBytes = 0;           // device bytes of the loaded IRs
		CabEntry* host[kTables] = {};     // pinned
		CabEntry* dev[kTables] = {};
		hipEvent_t done[kTables] = {};    // the launches that read dev[i] (and the upload that read host[i]) are over
		bool used[kTables] = {};
		int next = 0;
		int capacity = 0;                 // entries per table
		~CabinetStage();
	};
	hipError_t LaunchCabinetStage(const CabLaunch& L, hipStream_t stream); // (cabinet_stage_kernels.hip) the two launches of one piece

	bool HostDirect(); // (gpu_batch_host.cpp) the kernels read / write pinned host blocks themselves instead of the copy engines
}
