// compressor_stage.cpp -- the batch's side of the compressor stage (gpu_batch.h, compressor_stage.h): the rules of the
// calls, the lifetime of the curve and state blocks and the tables, and the one upload + one launch a processing call with entries
// enqueues.  The arithmetic and the bookkeeping are in compressor_stage.h; the stage's place in the chain is GpuBatch::StageId
// (gpu_batch.h), what every stage shares is in gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	namespace
	{
		constexpr size_t kCompCurveRowFloats = 2 * sizeof(CompCurve) / sizeof(float);
		constexpr size_t kCompStateRowFloats = sizeof(CompState) / sizeof(float);
	}

	GpuBatch::CompressorStage::~CompressorStage()
	{
		if (curves) (void)CountedHipFree(curves);
		if (state) (void)CountedHipFree(state);
	}

	void GpuBatch::EnableCompressorStage() { EnableStage<CompressorStage>(); }

	// set-up side (EnableCompressorStage, CreateStreams): two curve slots and a state per row, tables that hold what every row can put
	// into one call -- its entry and the curves of both slots
	void GpuBatch::CompressorStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want * kCompRowEntries);
		if (want > rowCapacity)
		{
			// the rows that exist keep their slots: whatever reads or writes the old blocks is over before they are copied
			if (state) batch.Quiesce();
			batch.GrowRowBlock(curves, kCompCurveRowFloats, rowCapacity, want, "hipMalloc (compressor curves)", "compressor curves");
			batch.GrowRowBlock(state, kCompStateRowFloats, rowCapacity, want, "hipMalloc (compressor state)", "compressor state");
			rowCapacity = want;
		}
	}

	CompressorStageInfo GpuBatch::GetCompressorInfo() const
	{
		const CompressorStage& st = Require<CompressorStage>("GetCompressorInfo");
		CompressorStageInfo info;
		info.curvePoints = kCompCurvePoints;
		info.numCompressors = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * (long long)((kCompCurveRowFloats + kCompStateRowFloats) * sizeof(float)) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamCompressor(int s, const CompParams* params, int fadeSamples)
	{
		CompBook& book = SettableStage<CompressorStage>(s, "SetStreamCompressor").book;
		if (params)
		{
			const std::string why = CompParamsError(*params);
			if (!why.empty()) throw std::runtime_error("neuralaudio_amd: SetStreamCompressor: " + why);
		}
		RequireFadeRange(fadeSamples, "SetStreamCompressor", "fadeSamples");
		if (book.Fading(s))
			throw std::runtime_error("neuralaudio_amd: SetStreamCompressor: a compressor fade of " + StreamId(s) + " is running (" + std::to_string(book.FadeRemaining(s)) + " samples left)");
		book.Set(s, params, fadeSamples);
	}

	bool GpuBatch::GetStreamCompressor(int s, CompParams& out) const
	{
		const CompressorStage& st = Require<CompressorStage>("GetStreamCompressor");
		RequireRow(s, "GetStreamCompressor");
		if (!st.book.HasCompressor(s)) return false;
		st.book.Target(s, out);
		return true;
	}

	int GpuBatch::StreamCompressorFadeRemaining(int s) const
	{
		const CompressorStage& st = Require<CompressorStage>("StreamCompressorFadeRemaining");
		RequireRow(s, "StreamCompressorFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// a diagnostic: the g of the last sample produced, from the state on the device
	float GpuBatch::StreamCompressorGain(int s)
	{
		CheckUsable();
		CompressorStage& st = Require<CompressorStage>("StreamCompressorGain");
		RequireRow(s, "StreamCompressorGain");
		if (!st.book.IsEntry(s) || st.book.Starting(s)) return 1.0f; // (no sample produced yet: it comes from the unity curve)
		Quiesce();
		CompState state;
		CheckHip(hipMemcpyAsync(&state, st.state + (size_t)s * kCompStateRowFloats, sizeof(CompState), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
		WaitStreamBounded(stream, "hipStreamSynchronize");
		return state.g;
	}

	// Behind the cabinet stage and in front of the delay stage, on the stream the model launches ran on: the table of this call's
	// entries -- and behind them the curves of the set calls since the last call: `units`, not `count`, go up -- from the next pinned
	// table of the ring (the wait for the launch that read it is bounded), ONE launch runs every entry over the call, and the host
	// mirror moves on by the n samples the caller sees.
	void GpuBatch::CompressorStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		if (n == 0) return;
		tables.Require(book.Rows() <= rowCapacity);
		const auto table = tables.Take(batch, book.NumEntries() * kCompRowEntries);
		int units = 0;
		const int count = book.BuildTable(table.host, units);
		if (count > 0)
		{
			tables.Upload(table, units, launch);
			CheckHip(LaunchCompressorStage(CompLaunch{ table.dev, count, dOut, outStride, (unsigned long long)n, reinterpret_cast<CompCurve*>(curves), reinterpret_cast<CompState*>(state) }, launch),
				"CompressorStageKernel");
			tables.Commit(launch);
		}
		book.Advance(n);
	}

	void GpuBatch::DebugRunCompressorStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		DebugRunStage(Require<CompressorStage>("DebugRunCompressorStage"), "DebugRunCompressorStage", hostRows, stride, n);
	}
}
