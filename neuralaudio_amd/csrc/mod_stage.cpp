// mod_stage.cpp -- the batch's side of the modulation stage (gpu_batch.h, mod_stage.h): the rules of the calls, the
// lifetime of rings and tables, and the one upload + one launch per piece a processing call with entries enqueues.  The arithmetic and
// the bookkeeping are in mod_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what every stage shares is in
// gpu_batch_internal.h.
#include <cmath>

#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::ModStage::~ModStage()
	{
		if (rings) (void)CountedHipFree(rings);
	}

	void GpuBatch::EnableModStage(int maxDelaySamples)
	{
		CheckUsable();
		if (maxDelaySamples < kModMinDelaySamples || maxDelaySamples > kModMaxDelaySamples) throw std::runtime_error("neuralaudio_amd: EnableModStage: maxDelaySamples must lie in [8, 4096]");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!stages[kModStage]) stages[kModStage].reset(new ModStage());
		ModStage& st = Require<ModStage>("EnableModStage");
		if (maxDelaySamples > st.book.MaxDelay())
		{
			if (st.book.HasEntries()) throw std::runtime_error("neuralaudio_amd: EnableModStage: a larger maxDelaySamples is refused while a stream has a modulation");
			if (ModBook::RingFor(maxDelaySamples) != st.book.RingSamples() && st.rings)
			{
				// (no stream has a modulation: no history to carry over; the launches that read the old rings are over before they go)
				Quiesce();
				(void)CountedHipFree(st.rings);
				st.rings = nullptr;
				st.ringRows = 0;
			}
			st.book.Configure(maxDelaySamples);
		}
		EnableStage<ModStage>();
	}

	// set-up side (EnableModStage, CreateStreams): a ring per row, tables that hold an entry per row
	void GpuBatch::ModStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want);
		if (want > ringRows)
		{
			// the rows that exist keep their histories: whatever reads or writes the old block is over before it is copied
			if (rings) batch.Quiesce();
			batch.GrowRowBlock(rings, (size_t)book.RingSamples(), ringRows, want, "hipMalloc (modulation rings)", "modulation rings");
			ringRows = want;
		}
	}

	ModStageInfo GpuBatch::GetModInfo() const
	{
		const ModStage& st = Require<ModStage>("GetModInfo");
		ModStageInfo info;
		info.maxDelaySamples = st.book.MaxDelay();
		info.ringSamples = st.book.RingSamples();
		info.pieceSamples = kModPieceSamples;
		info.numMods = st.book.NumEntries();
		info.deviceBytes = (long long)st.ringRows * st.book.RingSamples() * (long long)sizeof(float) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamMod(int s, const ModParams* params, int fadeSamples)
	{
		ModBook& book = SettableStage<ModStage>(s, "SetStreamMod").book;
		if (params)
			if (const char* why = ModParamsError(*params, book.MaxDelay()))
				throw std::runtime_error(std::string("neuralaudio_amd: SetStreamMod: ") + why + " (maxDelaySamples = " + std::to_string(book.MaxDelay()) + ")");
		RequireFadeRange(fadeSamples, "SetStreamMod", "fadeSamples");
		if (book.Fading(s))
			throw std::runtime_error("neuralaudio_amd: SetStreamMod: a modulation fade of " + StreamId(s) + " is running (" + std::to_string(book.FadeRemaining(s)) + " samples left)");
		if (params)
		{
			const int clash = book.PhaseClash(s, *params);
			if (clash >= 0) throw std::runtime_error("neuralaudio_amd: SetStreamMod: voicePhase[" + std::to_string(clash) + "] of a sounding voice must not change (" + StreamId(s) + ")");
		}
		book.Set(s, params, fadeSamples);
	}

	bool GpuBatch::GetStreamMod(int s, ModParams& out) const
	{
		const ModStage& st = Require<ModStage>("GetStreamMod");
		RequireRow(s, "GetStreamMod");
		if (!st.book.HasMod(s)) return false;
		out = st.book.Target(s);
		return true;
	}

	int GpuBatch::StreamModFadeRemaining(int s) const
	{
		const ModStage& st = Require<ModStage>("StreamModFadeRemaining");
		RequireRow(s, "StreamModFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// Behind the compressor stage and in front of the delay stage, on the stream the models ran on: the table of this call's entries goes
	// up from the next pinned table of the ring (the wait for the launch that read it is bounded), every piece of the call is one launch,
	// and the host mirror moves on by the n samples the caller sees.
	void GpuBatch::ModStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		tables.Require(book.Rows() <= ringRows);
		const auto table = tables.Take(batch, book.NumEntries());
		const int count = book.BuildTable(table.host);
		if (count > 0)
		{
			tables.Upload(table, count, launch);
			for (size_t done = 0; done < n; done += (size_t)kModPieceSamples)
			{
				const int piece = (int)std::min<size_t>((size_t)kModPieceSamples, n - done);
				CheckHip(LaunchModStage(ModLaunch{ table.dev, count, dOut, outStride, (unsigned long long)done, piece, rings, book.RingSamples() }, launch), "ModStageKernel");
			}
			tables.Commit(launch);
		}
		book.Advance(n);
	}

	void GpuBatch::DebugRunModStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		DebugRunStage(Require<ModStage>("DebugRunModStage"), "DebugRunModStage", hostRows, stride, n);
	}
}
