// gate_stage.cpp -- the batch's side of the gate stage (gpu_batch.h, gate_stage.h): the rules of the calls, the lifetime
// of the state and gain blocks and the tables, and the one upload + two launches a processing call with entries enqueues.  The
// arithmetic and the bookkeeping are in gate_stage.h.
#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::GateStage::~GateStage()
	{
		if (state) (void)CountedHipFree(state);
		if (gains) (void)CountedHipFree(gains);
	}

	void GpuBatch::EnableGateStage()
	{
		CheckUsable();
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!gateStage) gateStage.reset(new GateStage());
		EnsureGateRows((int)streams.size());
		EnsurePoolPipeline(); // (an entry moves Submit's buffers onto the slots' own streams or the copy streams: they exist from here on)
	}

	// set-up side (EnableGateStage, CreateStreams): a state and a gain row per row, tables that hold an entry per row
	void GpuBatch::EnsureGateRows(int rows)
	{
		GateStage& st = *gateStage;
		st.book.Resize(rows);
		const int want = std::max(rows, 16);
		st.tables.Ensure(*this, want);
		if (want > st.rowCapacity)
		{
			// the rows that exist keep their states: whatever reads or writes the old blocks is over before they are copied
			if (st.state) Quiesce();
			static_assert(sizeof(GateState) == 4 * sizeof(float), "a state row is four words");
			GrowRowBlock(st.state, sizeof(GateState) / sizeof(float), st.rowCapacity, want, "hipMalloc (gate state)", "gate state");
			GrowRowBlock(st.gains, (size_t)st.gainSamples, 0, want, "hipMalloc (gate gains)", "gate gains"); // (nothing of a gain row outlives its call)
			st.rowCapacity = want;
		}
	}

	// a call longer than the gain rows: they grow (not real-time safe, like any first use of a longer buffer)
	void GpuBatch::EnsureGateSamples(size_t n)
	{
		GateStage& st = *gateStage;
		if (n <= (size_t)st.gainSamples) return;
		if (n > (size_t)1 << 30) throw std::runtime_error("neuralaudio_amd: gate stage: the call is too long for the gain block");
		int samples = st.gainSamples;
		while ((size_t)samples < n) samples *= 2;
		Quiesce(); // (the apply launch of an earlier call may still read the old block)
		GrowRowBlock(st.gains, (size_t)samples, 0, st.rowCapacity, "hipMalloc (gate gains)", "gate gains");
		st.gainSamples = samples;
	}

	GateStageInfo GpuBatch::GetGateInfo() const
	{
		const GateStage& st = RequireStage(gateStage, "GetGateInfo");
		GateStageInfo info;
		info.gainSamples = st.gainSamples;
		info.numGates = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * ((long long)st.gainSamples * (long long)sizeof(float) + (long long)sizeof(GateState)) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamGate(int s, const GateParams* params, bool startOpen)
	{
		CheckUsable();
		GateBook& book = RequireStage(gateStage, "SetStreamGate").book;
		if (IsParked(s)) throw std::runtime_error("neuralaudio_amd: SetStreamGate: " + StreamId(s) + " is parked");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: SetStreamGate: " + StreamId(s) + " is not a live stream of the batch");
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
		const GateStage& st = RequireStage(gateStage, "GetStreamGate");
		RequireRow(s, "GetStreamGate");
		if (!st.book.HasGate(s)) return false;
		out = st.book.Params(s);
		return true;
	}

	// a diagnostic: the g of the last sample produced, from the state on the device
	float GpuBatch::StreamGateGain(int s)
	{
		CheckUsable();
		GateStage& st = RequireStage(gateStage, "StreamGateGain");
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

	// The stream leaves (ParkStream, RemoveStreams): its gate goes at once -- a parked stream carries nothing over
	void GpuBatch::GateLeave(int s)
	{
		if (!gateStage || s >= gateStage->book.Rows()) return;
		gateStage->book.Leave(s);
	}

	// In front of everything else of the call, on the stream it runs on: the table of this call's entries goes up from the next pinned
	// table of the ring (the wait for the launch that read it is bounded) and the detector reads the input rows as the caller passed
	// them -- they may be the output rows -- into the gain block.
	void GpuBatch::RunGateDetector(hipStream_t launch, const float* dIn, size_t n, long inStride)
	{
		GateStage& st = *gateStage;
		st.count = 0;
		if (st.book.NumEntries() > st.tables.capacity || st.book.Rows() > st.rowCapacity) throw std::runtime_error("neuralaudio_amd: gate stage: more entries than the tables hold");
		EnsureGateSamples(n);
		const auto table = st.tables.Take(*this);
		const int count = st.book.BuildTable(table.host);
		if (count == 0) return;
		CheckHip(hipMemcpyAsync(table.dev, table.host, (size_t)count * sizeof(GateEntry), hipMemcpyHostToDevice, launch), "hipMemcpyAsync (gate stage table)");
		CheckHip(LaunchGateDetect(GateDetectLaunch{ table.dev, count, dIn, inStride, (unsigned long long)n, st.gains, (long)st.gainSamples, reinterpret_cast<GateState*>(st.state) }, launch),
			"GateDetectKernel");
		st.count = count;
		st.dev = table.dev;
	}

	// Behind the model launches (behind the down kernel of a resampling batch), first of the stages: the rows of the entries the
	// detector saw are scaled in place, the table's ring moves on and the host mirror by the n samples the caller sees.
	void GpuBatch::RunGateApply(hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		GateStage& st = *gateStage;
		if (st.count == 0) return;
		CheckHip(LaunchGateApply(GateApplyLaunch{ st.dev, st.count, dOut, outStride, (unsigned long long)n, st.gains, (long)st.gainSamples }, launch), "GateApplyKernel");
		st.tables.Commit(launch);
		st.count = 0;
		st.book.Advance(n);
	}
}
