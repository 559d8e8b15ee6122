// eq_stage.cpp -- the batch's side of the EQ stage (gpu_batch.h, eq_stage.h): the rules of the calls, the lifetime of
// the coefficient and state blocks and the tables, and the one upload + one launch a processing call with entries enqueues.  The
// arithmetic and the bookkeeping are in eq_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what every stage
// shares is in gpu_batch_internal.h.
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

	void GpuBatch::EnableEqStage() { EnableStage<EqStage>(); }

	// set-up side (EnableEqStage, CreateStreams): two slots per row, tables that hold what every row can put into one call -- its entry
	// and the coefficient sets of both slots
	void GpuBatch::EqStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want * kEqRowEntries);
		if (want > rowCapacity)
		{
			// the rows that exist keep their slots: whatever reads or writes the old blocks is over before they are copied
			if (state) batch.Quiesce();
			batch.GrowRowBlock(coefs, kEqCoefRowFloats, rowCapacity, want, "hipMalloc (eq coefficients)", "eq coefficients");
			batch.GrowRowBlock(state, kEqStateRowFloats, rowCapacity, want, "hipMalloc (eq state)", "eq state");
			rowCapacity = want;
		}
	}

	EqStageInfo GpuBatch::GetEqInfo() const
	{
		const EqStage& st = Require<EqStage>("GetEqInfo");
		EqStageInfo info;
		info.maxSections = kEqMaxSections;
		info.numEntries = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * (long long)((kEqCoefRowFloats + kEqStateRowFloats) * sizeof(float)) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamEq(int s, const EqSection* sections, int numSections, int fadeSamples)
	{
		EqBook& book = SettableStage<EqStage>(s, "SetStreamEq").book;
		const std::string why = EqSectionsError(sections, numSections);
		if (!why.empty()) throw std::runtime_error("neuralaudio_amd: SetStreamEq: " + why);
		RequireFadeRange(fadeSamples, "SetStreamEq", "fadeSamples");
		if (book.Fading(s)) throw std::runtime_error("neuralaudio_amd: SetStreamEq: an EQ fade of " + StreamId(s) + " is running");
		book.Set(s, sections, numSections, fadeSamples);
	}

	int GpuBatch::GetStreamEq(int s, EqSection* out, int capacity) const
	{
		const EqStage& st = Require<EqStage>("GetStreamEq");
		RequireRow(s, "GetStreamEq");
		return st.book.Target(s, out, out ? std::max(capacity, 0) : 0);
	}

	int GpuBatch::StreamEqFadeRemaining(int s) const
	{
		const EqStage& st = Require<EqStage>("StreamEqFadeRemaining");
		RequireRow(s, "StreamEqFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// Behind the gate's apply and in front of the cabinet stage, on the stream the model launches ran on: the table of this call's
	// entries -- and behind them the coefficients of the set calls since the last call: `units`, not `count`, go up -- from the next
	// pinned table of the ring (the wait for the launch that read it is bounded), ONE launch runs every entry's cascade over the call,
	// and the host mirror moves on by the n samples the caller sees.
	void GpuBatch::EqStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		if (n == 0) return;
		tables.Require(book.Rows() <= rowCapacity);
		const auto table = tables.Take(batch, book.NumEntries() * kEqRowEntries);
		int units = 0;
		const int count = book.BuildTable(table.host, units);
		if (count > 0)
		{
			tables.Upload(table, units, launch);
			CheckHip(LaunchEqStage(EqLaunch{ table.dev, count, dOut, outStride, (unsigned long long)n, reinterpret_cast<EqCoefSet*>(coefs), reinterpret_cast<EqSecState*>(state) }, launch),
				"EqStageKernel");
			tables.Commit(launch);
		}
		book.Advance(n);
	}

	void GpuBatch::DebugRunEqStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		DebugRunStage(Require<EqStage>("DebugRunEqStage"), "DebugRunEqStage", hostRows, stride, n);
	}
}
