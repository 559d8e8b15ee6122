// gate_stage.cpp -- the batch's side of the gate stage (gpu_batch.h, gate_stage.h): the rules of the calls, the lifetime
// of the state and gain blocks and the tables, and the one upload + two launches a processing call with entries enqueues.  The
// arithmetic and the bookkeeping are in gate_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what every
// stage shares is in gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::GateStage::~GateStage()
	{
		if (state) (void)CountedHipFree(state);
		if (gains) (void)CountedHipFree(gains);
	}

	void GpuBatch::EnableGateStage() { EnableStage<GateStage>(); }

	// set-up side (EnableGateStage, CreateStreams): a state and a gain row per row, tables that hold an entry per row
	void GpuBatch::GateStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want);
		if (want > rowCapacity)
		{
			// the rows that exist keep their states: whatever reads or writes the old blocks is over before they are copied
			if (state) batch.Quiesce();
			static_assert(sizeof(GateState) == 4 * sizeof(float), "a state row is four words");
			batch.GrowRowBlock(state, sizeof(GateState) / sizeof(float), rowCapacity, want, "hipMalloc (gate state)", "gate state");
			batch.GrowRowBlock(gains, (size_t)gainSamples, 0, want, "hipMalloc (gate gains)", "gate gains"); // (nothing of a gain row outlives its call)
			rowCapacity = want;
		}
	}

	// a call longer than the gain rows: they grow (not real-time safe, like any first use of a longer buffer)
	void GpuBatch::GateStage::EnsureSamples(GpuBatch& batch, size_t n)
	{
		if (n <= (size_t)gainSamples) return;
		if (n > (size_t)1 << 30) throw std::runtime_error("neuralaudio_amd: gate stage: the call is too long for the gain block");
		int samples = gainSamples;
		while ((size_t)samples < n) samples *= 2;
		batch.Quiesce(); // (the apply launch of an earlier call may still read the old block)
		batch.GrowRowBlock(gains, (size_t)samples, 0, rowCapacity, "hipMalloc (gate gains)", "gate gains");
		gainSamples = samples;
	}

	GateStageInfo GpuBatch::GetGateInfo() const
	{
		const GateStage& st = Require<GateStage>("GetGateInfo");
		GateStageInfo info;
		info.gainSamples = st.gainSamples;
		info.numGates = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * ((long long)st.gainSamples * (long long)sizeof(float) + (long long)sizeof(GateState)) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamGate(int s, const GateParams* params, bool startOpen)
	{
		GateBook& book = SettableStage<GateStage>(s, "SetStreamGate").book;
		if (!params)
		{
			book.Remove(s);
			return;
		}
		if (const char* why = GateParamsError(*params)) throw std::runtime_error(std::string("neuralaudio_amd: SetStreamGate: ") + why);
		book.Set(s, *params, startOpen);
	}

	bool GpuBatch::GetStreamGate(int s, GateParams& out) const
	{
		const GateStage& st = Require<GateStage>("GetStreamGate");
		RequireRow(s, "GetStreamGate");
		if (!st.book.HasGate(s)) return false;
		out = st.book.Params(s);
		return true;
	}

	// a diagnostic: the g of the last sample produced, from the state on the device
	float GpuBatch::StreamGateGain(int s)
	{
		CheckUsable();
		GateStage& st = Require<GateStage>("StreamGateGain");
		RequireRow(s, "StreamGateGain");
		if (!st.book.IsEntry(s)) return 1.0f;
		const GateConsts c = GateConstsOf(st.book.Params(s));
		if (st.book.Start(s) == kGateStartOpen) return 1.0f; // (no sample produced yet: what the gate starts from)
		if (st.book.Start(s) == kGateStartClosed) return c.floor;
		Quiesce();
		GateState state;
		CheckHip(hipMemcpyAsync(&state, st.state + (size_t)s * (sizeof(GateState) / sizeof(float)), sizeof(GateState), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
		WaitStreamBounded(stream, "hipStreamSynchronize");
		return GateGainOf(c, state.u);
	}

	// In front of everything else of the call, on the stream it runs on: the table of this call's entries goes up from the next pinned
	// table of the ring (the wait for the launch that read it is bounded) and the detector reads the input rows as the caller passed
	// them -- they may be the output rows -- into the gain block.
	void GpuBatch::GateStage::BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride)
	{
		count = 0;
		tables.Require(book.Rows() <= rowCapacity);
		EnsureSamples(batch, n);
		const auto table = tables.Take(batch, book.NumEntries());
		const int entries = book.BuildTable(table.host);
		if (entries == 0) return;
		tables.Upload(table, entries, launch);
		CheckHip(LaunchGateDetect(GateDetectLaunch{ table.dev, entries, dIn, inStride, (unsigned long long)n, gains, (long)gainSamples, reinterpret_cast<GateState*>(state) }, launch),
			"GateDetectKernel");
		count = entries;
		dev = table.dev;
	}

	// Behind the model launches (behind the down kernel of a resampling batch), first of the stages: the rows of the entries the
	// detector saw are scaled in place, the table's ring moves on and the host mirror by the n samples the caller sees.
	void GpuBatch::GateStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		(void)batch;
		if (count == 0) return;
		CheckHip(LaunchGateApply(GateApplyLaunch{ dev, count, dOut, outStride, (unsigned long long)n, gains, (long)gainSamples }, launch), "GateApplyKernel");
		tables.Commit(launch);
		count = 0;
		book.Advance(n);
	}
}
