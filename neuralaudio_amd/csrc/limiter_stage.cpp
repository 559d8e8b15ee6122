// limiter_stage.cpp -- the batch's side of the limiter stage (gpu_batch.h, limiter_stage.h): the rules of the calls,
// the lifetime of the history rings and the tables, and the one upload + one launch per piece a processing call with entries enqueues.
// The arithmetic and the bookkeeping are in limiter_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what
// every stage shares is in gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::LimiterStage::~LimiterStage()
	{
		if (history) (void)CountedHipFree(history);
	}

	void GpuBatch::EnableLimiterStage()
	{
		CheckUsable();
		if (Resamples()) throw std::runtime_error("neuralaudio_amd: EnableLimiterStage: the limiter stage is refused on a resampling batch");
		EnableStage<LimiterStage>();
	}

	// set-up side (EnableLimiterStage, CreateStreams): a history ring per row, tables that hold an entry per row
	void GpuBatch::LimiterStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want);
		if (want > rowCapacity)
		{
			// the rows that exist keep their histories: whatever reads or writes the old block is over before it is copied
			if (history) batch.Quiesce();
			batch.GrowRowBlock(history, (size_t)kLimHistory, rowCapacity, want, "hipMalloc (limiter history)", "limiter history");
			rowCapacity = want;
		}
	}

	LimiterStageInfo GpuBatch::GetLimiterInfo() const
	{
		const LimiterStage& st = Require<LimiterStage>("GetLimiterInfo");
		LimiterStageInfo info;
		info.historySamples = kLimHistory;
		info.pieceSamples = kLimPieceSamples;
		info.numLimiters = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * kLimHistory * (long long)sizeof(float) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamLimiter(int s, const LimiterParams* params, int rampSamples)
	{
		LimiterBook& book = SettableStage<LimiterStage>(s, "SetStreamLimiter").book;
		if (!params)
		{
			book.Remove(s);
			return;
		}
		if (const char* why = LimiterParamsError(*params)) throw std::runtime_error(std::string("neuralaudio_amd: SetStreamLimiter: ") + why);
		RequireFadeRange(rampSamples, "SetStreamLimiter", "rampSamples");
		if (book.HasLimiter(s) && book.Target(s).lookahead != params->lookahead)
			throw std::runtime_error("neuralaudio_amd: SetStreamLimiter: lookahead belongs to the limiter for its life (" + StreamId(s) + " has one: take it away first)");
		book.Set(s, *params, rampSamples);
	}

	bool GpuBatch::GetStreamLimiter(int s, LimiterParams& out) const
	{
		const LimiterStage& st = Require<LimiterStage>("GetStreamLimiter");
		RequireRow(s, "GetStreamLimiter");
		if (!st.book.HasLimiter(s)) return false;
		out = st.book.Target(s);
		return true;
	}

	// Behind the mix stage and in front of the meter's OUT tap, on the stream the models ran on: the table of this call's entries goes up
	// from the next pinned table of the ring (the wait for the launch that read it is bounded), every piece of the call is one launch --
	// in order, so no two workgroups touch a row at once --, and the host mirror moves on by the n samples the caller sees.
	void GpuBatch::LimiterStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		tables.Require(book.Rows() <= rowCapacity);
		const auto table = tables.Take(batch, book.NumEntries());
		int maxWindow = 0, maxLookahead = 0;
		const int count = book.BuildTable(table.host, maxWindow, maxLookahead);
		if (count > 0)
		{
			tables.Upload(table, count, launch);
			for (size_t done = 0; done < n; done += (size_t)kLimPieceSamples)
			{
				const int piece = (int)std::min<size_t>((size_t)kLimPieceSamples, n - done);
				CheckHip(LaunchLimiterStage(LimiterLaunch{ table.dev, count, dOut, outStride, (unsigned long long)done, piece, history, rowCapacity, maxWindow, maxLookahead }, launch),
					"LimiterStageKernel");
			}
			tables.Commit(launch);
		}
		book.Advance(n);
	}
}
