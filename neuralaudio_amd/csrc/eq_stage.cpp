// eq_stage.cpp -- the batch's side of the EQ stage (gpu_batch.h, eq_stage.h): the rules of the calls, the lifetime of
// the coefficient and state blocks and the tables, and the one upload + one launch a processing call with entries enqueues.  The
// arithmetic and the bookkeeping are in eq_stage.h.
#include "gpu_batch_internal.h"

namespace na
{
	namespace
	{
		constexpr size_t kEqCoefRowFloats = 2 * sizeof(EqCoefSet) / sizeof(float);
		constexpr size_t kEqStateRowFloats = 2 * kEqMaxSections * sizeof(EqSecState) / sizeof(float);
	}

	GpuBatch::EqStage::~EqStage()
	{
		if (coefs) (void)CountedHipFree(coefs);
		if (state) (void)CountedHipFree(state);
	}

	void GpuBatch::EnableEqStage()
	{
		CheckUsable();
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!eqStage) eqStage.reset(new EqStage());
		EnsureEqRows((int)streams.size());
		EnsurePoolPipeline(); // (an entry moves Submit's buffers onto the slots' own streams or the copy streams: they exist from here on)
	}

	// set-up side (EnableEqStage, CreateStreams): two slots per row, tables that hold what every row can put into one call -- its entry
	// and the coefficient sets of both slots
	void GpuBatch::EnsureEqRows(int rows)
	{
		EqStage& st = *eqStage;
		st.book.Resize(rows);
		const int want = std::max(rows, 16);
		st.tables.Ensure(*this, want * kEqRowEntries);
		if (want > st.rowCapacity)
		{
			// the rows that exist keep their slots: whatever reads or writes the old blocks is over before they are copied
			if (st.state) Quiesce();
			GrowRowBlock(st.coefs, kEqCoefRowFloats, st.rowCapacity, want, "hipMalloc (eq coefficients)", "eq coefficients");
			GrowRowBlock(st.state, kEqStateRowFloats, st.rowCapacity, want, "hipMalloc (eq state)", "eq state");
			st.rowCapacity = want;
		}
	}

	EqStageInfo GpuBatch::GetEqInfo() const
	{
		const EqStage& st = RequireStage(eqStage, "GetEqInfo");
		EqStageInfo info;
		info.maxSections = kEqMaxSections;
		info.numEntries = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * (long long)((kEqCoefRowFloats + kEqStateRowFloats) * sizeof(float)) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamEq(int s, const EqSection* sections, int numSections, int fadeSamples)
	{
		CheckUsable();
		EqBook& book = RequireStage(eqStage, "SetStreamEq").book;
		if (IsParked(s)) throw std::runtime_error("neuralaudio_amd: SetStreamEq: " + StreamId(s) + " is parked");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: SetStreamEq: " + StreamId(s) + " is not a live stream of the batch");
		const std::string why = EqSectionsError(sections, numSections);
		if (!why.empty()) throw std::runtime_error("neuralaudio_amd: SetStreamEq: " + why);
		if (fadeSamples < 0 || fadeSamples > kOutStageMaxRamp) throw std::runtime_error("neuralaudio_amd: SetStreamEq: fadeSamples must lie in [0, 1 << 20]");
		if (book.Fading(s)) throw std::runtime_error("neuralaudio_amd: SetStreamEq: an EQ fade of " + StreamId(s) + " is running");
		book.Set(s, sections, numSections, fadeSamples);
	}

	int GpuBatch::GetStreamEq(int s, EqSection* out, int capacity) const
	{
		const EqStage& st = RequireStage(eqStage, "GetStreamEq");
		RequireRow(s, "GetStreamEq");
		return st.book.Target(s, out, out ? std::max(capacity, 0) : 0);
	}

	int GpuBatch::StreamEqFadeRemaining(int s) const
	{
		const EqStage& st = RequireStage(eqStage, "StreamEqFadeRemaining");
		RequireRow(s, "StreamEqFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// The stream leaves (ParkStream, RemoveStreams): flat at once, its states dropped -- a parked stream carries nothing over
	void GpuBatch::EqLeave(int s)
	{
		if (!eqStage || s >= eqStage->book.Rows()) return;
		eqStage->book.Leave(s);
	}

	// Behind the gate's apply and in front of the cabinet stage, on the stream the model launches ran on: the table of this call's
	// entries -- and behind them the coefficients of the set calls since the last call -- goes up from the next pinned table of the ring
	// (the wait for the launch that read it is bounded), ONE launch runs every entry's cascade over the call, and the host mirror moves
	// on by the n samples the caller sees.
	void GpuBatch::RunEqStage(hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		EqStage& st = *eqStage;
		if (n == 0) return;
		if (st.book.NumEntries() * kEqRowEntries > st.tables.capacity || st.book.Rows() > st.rowCapacity) throw std::runtime_error("neuralaudio_amd: eq stage: more entries than the tables hold");
		const auto table = st.tables.Take(*this);
		int units = 0;
		const int count = st.book.BuildTable(table.host, units);
		if (count > 0)
		{
			CheckHip(hipMemcpyAsync(table.dev, table.host, (size_t)units * sizeof(EqEntry), hipMemcpyHostToDevice, launch), "hipMemcpyAsync (eq stage table)");
			CheckHip(LaunchEqStage(EqLaunch{ table.dev, count, dOut, outStride, (unsigned long long)n, reinterpret_cast<EqCoefSet*>(st.coefs), reinterpret_cast<EqSecState*>(st.state) }, launch),
				"EqStageKernel");
			st.tables.Commit(launch);
		}
		st.book.Advance(n);
	}

	// test hook (NA_DebugRunEqStage): what a processing call of n samples runs for the stage, on host rows in place of model outputs
	void GpuBatch::DebugRunEqStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		const EqStage& st = RequireStage(eqStage, "DebugRunEqStage");
		if (!hostRows || n == 0 || stride < (long)n || streams.empty()) throw std::runtime_error("neuralaudio_amd: DebugRunEqStage: bad argument");
		Quiesce();
		if (!st.book.HasEntries()) return;
		const size_t floats = (size_t)streams.size() * (size_t)stride;
		float* dRows = nullptr;
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dRows), floats * sizeof(float)), "hipMalloc");
		try
		{
			CheckHip(hipMemcpyAsync(dRows, hostRows, floats * sizeof(float), hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
			RunEqStage(stream, dRows, n, stride);
			CheckHip(hipMemcpyAsync(hostRows, dRows, floats * sizeof(float), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
			WaitStreamBounded(stream, "hipStreamSynchronize");
		}
		catch (...)
		{
			if (!broken) (void)CountedHipFree(dRows);
			throw;
		}
		(void)CountedHipFree(dRows);
	}
}
