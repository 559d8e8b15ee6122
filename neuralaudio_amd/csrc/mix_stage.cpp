// mix_stage.cpp -- the batch's side of the mix stage (gpu_batch.h, mix_stage.h): the rules of the calls, the lifetime of
// the matrix and stash blocks and the tables, and the one upload + one launch (+ one stash launch) a processing call with groups
// enqueues.  The arithmetic and the bookkeeping are in mix_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h),
// what every stage shares is in gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::MixStage::~MixStage()
	{
		if (gains) (void)CountedHipFree(gains);
		if (stash) (void)CountedHipFree(stash);
	}

	void GpuBatch::EnableMixStage() { EnableStage<MixStage>(); }

	// set-up side (EnableMixStage, CreateStreams): two matrices and a stash row per row, tables that hold what every row can put into
	// one call -- a group's entry and its gain set (a group has a first member, so there are no more groups than rows)
	void GpuBatch::MixStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want * kMixRowEntries);
		if (want > rowCapacity)
		{
			// the groups that exist keep their matrices: whatever reads or writes the old blocks is over before they are copied
			if (gains) batch.Quiesce();
			batch.GrowRowBlock(gains, (size_t)kMixSetFloats, rowCapacity, want, "hipMalloc (mix gains)", "mix gains");
			batch.GrowRowBlock(stash, (size_t)drySamples, 0, want, "hipMalloc (mix stash)", "mix stash"); // (nothing of a stash row outlives its call)
			rowCapacity = want;
		}
	}

	// a call with a DRY member longer than the stash rows: they grow (not real-time safe, like any first use of a longer buffer)
	void GpuBatch::MixStage::EnsureSamples(GpuBatch& batch, size_t n)
	{
		if (n <= (size_t)drySamples) return;
		if (n > (size_t)1 << 30) throw std::runtime_error("neuralaudio_amd: mix stage: the call is too long for the stash block");
		int samples = drySamples;
		while ((size_t)samples < n) samples *= 2;
		batch.Quiesce(); // (the mix launch of an earlier call may still read the old block)
		batch.GrowRowBlock(stash, (size_t)samples, 0, rowCapacity, "hipMalloc (mix stash)", "mix stash");
		drySamples = samples;
	}

	MixStageInfo GpuBatch::GetMixInfo() const
	{
		const MixStage& st = Require<MixStage>("GetMixInfo");
		MixStageInfo info;
		info.maxMembers = kMixMaxMembers;
		info.numGroups = st.book.NumGroups();
		info.drySamples = st.drySamples;
		info.deviceBytes = (long long)st.rowCapacity * ((long long)st.drySamples + kMixSetFloats) * (long long)sizeof(float) + st.tables.Bytes();
		return info;
	}

	bool GpuBatch::HasDryMixGroup() const
	{
		const Stage* stage = stages[kMixStage].get();
		return stage && static_cast<const MixStage&>(*stage).book.HasDry();
	}

	void GpuBatch::SetMixGroup(const int* ids, const int* taps, int M, int D, const float* gains, int rampSamples)
	{
		static const char* const who = "SetMixGroup";
		const std::string head = "neuralaudio_amd: SetMixGroup: ";
		CheckUsable();
		MixBook& book = Require<MixStage>(who).book;
		if (M < 1 || M > kMixMaxMembers) throw std::runtime_error(head + "numMembers must lie in [1, 8]");
		if (D < 1 || D > M) throw std::runtime_error(head + "numOutputs must lie in [1, numMembers]");
		if (!ids || !gains) throw std::runtime_error(head + "bad argument");
		bool dry = false;
		for (int j = 0; j < M; j++)
		{
			(void)SettableStage<MixStage>(ids[j], who); // live and not parked
			const int tap = taps ? taps[j] : kMixTapOut;
			if (tap != kMixTapOut && tap != kMixTapDry) throw std::runtime_error(head + "a tap must be NA_MIX_TAP_OUT or NA_MIX_TAP_DRY");
			dry = dry || tap == kMixTapDry;
		}
		for (int j = 0; j < M; j++)
			for (int i = 0; i < j; i++)
			{
				const bool sameTap = (taps ? taps[i] : kMixTapOut) == (taps ? taps[j] : kMixTapOut);
				if (ids[i] != ids[j]) continue;
				if (j < D) throw std::runtime_error(head + "the outputs must be OUT taps of distinct streams (" + StreamId(ids[j]) + " is named twice)");
				if (sameTap) throw std::runtime_error(head + "duplicate member: " + StreamId(ids[j]) + " appears twice in the same tap");
			}
		for (int d = 0; d < D; d++)
			if (taps && taps[d] != kMixTapOut) throw std::runtime_error(head + "the outputs must be OUT taps of distinct streams (member " + std::to_string(d) + " is a DRY tap)");
		for (int c = 0; c < D * M; c++)
			if (!std::isfinite(gains[c])) throw std::runtime_error(head + "every gain must be finite");
		RequireFadeRange(rampSamples, who, "rampSamples");
		const int first = book.GroupOf(ids[0]);
		if (!(first == ids[0] && book.Matches(first, ids, taps, M, D)))
		{
			for (int j = 0; j < M; j++)
				if (book.GroupOf(ids[j]) >= 0) throw std::runtime_error(head + StreamId(ids[j]) + " is already in another mix group");
			if (dry && Resamples())
				throw std::runtime_error(head + "a DRY tap is refused on a resampling batch (the rows lag the input by the resampler's latency: an unaligned dry blend is a comb filter)");
		}
		book.Set(ids, taps, M, D, gains, rampSamples);
	}

	void GpuBatch::ClearMixGroup(int s)
	{
		CheckUsable();
		MixBook& book = Require<MixStage>("ClearMixGroup").book;
		RequireRow(s, "ClearMixGroup");
		book.Leave(s);
	}

	int GpuBatch::GetStreamMix(int s, int* ids, int* taps, int capacity, int* numOutputs, float* gains) const
	{
		const MixBook& book = Require<MixStage>("GetStreamMix").book;
		RequireRow(s, "GetStreamMix");
		const int g = book.GroupOf(s);
		if (g < 0) return 0;
		const MixBook::Group& grp = book.At(g);
		for (int j = 0; j < std::min(grp.M, std::max(capacity, 0)); j++)
		{
			if (ids) ids[j] = grp.row[j];
			if (taps) taps[j] = grp.tap[j];
		}
		if (numOutputs) *numOutputs = grp.D;
		if (gains && capacity >= grp.M)
			for (int d = 0; d < grp.D; d++)
				for (int j = 0; j < grp.M; j++) gains[d * grp.M + j] = grp.g1[d * kMixMaxMembers + j];
		return grp.M;
	}

	int GpuBatch::MixRampRemaining(int s) const
	{
		const MixBook& book = Require<MixStage>("MixRampRemaining").book;
		RequireRow(s, "MixRampRemaining");
		const int g = book.GroupOf(s);
		return g < 0 ? 0 : book.RampRemaining(g);
	}

	// In front of the model launches, on the stream the call runs on: the table of this call's groups -- and behind them the matrices of
	// the set calls since the last call: `units`, not `count`, go up -- from the next pinned table of the ring (the wait for the launch
	// that read it is bounded), and, while some group has a DRY member, the stash launch reads those members' input rows as the caller
	// passed them -- they may be the output rows -- into the stash block.
	void GpuBatch::MixStage::BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride)
	{
		count = 0;
		if (n == 0) return;
		tables.Require(book.Rows() <= rowCapacity);
		if (book.HasDry()) EnsureSamples(batch, n);
		const auto table = tables.Take(batch, book.NumGroups() * kMixRowEntries);
		int units = 0;
		const int entries = book.BuildTable(table.host, units);
		if (entries == 0) return;
		tables.Upload(table, units, launch);
		if (book.HasDry())
		{
			if (!dIn) throw std::runtime_error("neuralaudio_amd: mix stage: a group has a DRY member and the call has no input rows");
			CheckHip(LaunchMixStash(MixStashLaunch{ table.dev, entries, dIn, inStride, (unsigned long long)n, stash, (long)drySamples }, launch), "MixStashKernel");
		}
		count = entries;
		dev = table.dev;
	}

	// Behind the output stage and in front of the meter's OUT tap: ONE launch mixes every group of the table in place, the table's ring
	// moves on and the host mirror by the n samples the caller sees.
	void GpuBatch::MixStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		(void)batch;
		if (count == 0) return;
		CheckHip(LaunchMixStage(MixLaunch{ dev, count, dOut, outStride, (unsigned long long)n, gains, stash, (long)drySamples }, launch), "MixStageKernel");
		tables.Commit(launch);
		count = 0;
		book.Advance(n);
	}

	void GpuBatch::DebugRunMixStage(const float* hostIn, float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		MixStage& st = Require<MixStage>("DebugRunMixStage");
		if (!hostIn && st.book.HasDry()) throw std::runtime_error("neuralaudio_amd: DebugRunMixStage: bad argument (a group has a DRY member: hostIn is needed)");
		DebugRunStage(st, "DebugRunMixStage", hostRows, stride, n, hostIn);
	}
}
