// delay_stage.cpp -- the batch's side of the delay stage (gpu_batch.h, delay_stage.h): the rules of the calls, the
// lifetime of rings, filter states and tables, and the one upload + one launch per piece a processing call with entries enqueues.  The
// arithmetic and the bookkeeping are in delay_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what every
// stage shares is in gpu_batch_internal.h.
#include <cmath>

#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::DelayStage::~DelayStage()
	{
		if (rings) (void)CountedHipFree(rings);
		if (state) (void)CountedHipFree(state);
	}

	void GpuBatch::EnableDelayStage(int maxDelaySamples)
	{
		CheckUsable();
		if (maxDelaySamples < 1 || maxDelaySamples > kDelayMaxSamples) throw std::runtime_error("neuralaudio_amd: EnableDelayStage: maxDelaySamples must lie in [1, 1 << 18]");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!stages[kDelayStage]) stages[kDelayStage].reset(new DelayStage());
		DelayStage& st = Require<DelayStage>("EnableDelayStage");
		if (maxDelaySamples > st.book.MaxDelay())
		{
			if (st.book.HasEntries()) throw std::runtime_error("neuralaudio_amd: EnableDelayStage: a larger maxDelaySamples is refused while a stream has a delay");
			if (DelayBook::RingFor(maxDelaySamples) != st.book.RingSamples() && st.rings)
			{
				// (no stream has a delay: no history to carry over; the launches that read the old rings are over before they go)
				Quiesce();
				(void)CountedHipFree(st.rings);
				st.rings = nullptr;
				st.ringRows = 0;
			}
			st.book.Configure(maxDelaySamples);
		}
		EnableStage<DelayStage>();
	}

	// set-up side (EnableDelayStage, CreateStreams): a ring and a filter state per row, tables that hold an entry per row
	void GpuBatch::DelayStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want);
		if (want > ringRows || want > stateRows)
		{
			// the rows that exist keep their histories: whatever reads or writes the old blocks is over before they are copied
			if (rings || state) batch.Quiesce();
			if (want > ringRows)
			{
				batch.GrowRowBlock(rings, (size_t)book.RingSamples(), ringRows, want, "hipMalloc (delay rings)", "delay rings");
				ringRows = want;
			}
			if (want > stateRows)
			{
				static_assert(sizeof(DelayFilter) == 2 * sizeof(float), "a state row is two words");
				batch.GrowRowBlock(state, sizeof(DelayFilter) / sizeof(float), stateRows, want, "hipMalloc (delay state)", "delay state");
				stateRows = want;
			}
		}
	}

	DelayStageInfo GpuBatch::GetDelayInfo() const
	{
		const DelayStage& st = Require<DelayStage>("GetDelayInfo");
		DelayStageInfo info;
		info.maxDelaySamples = st.book.MaxDelay();
		info.ringSamples = st.book.RingSamples();
		info.pieceSamples = kDelayPieceSamples;
		info.numDelays = st.book.NumEntries();
		info.deviceBytes = (long long)st.ringRows * st.book.RingSamples() * (long long)sizeof(float) + (long long)st.stateRows * (long long)sizeof(DelayFilter) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamDelay(int s, const DelayParams* params, int fadeSamples)
	{
		DelayBook& book = SettableStage<DelayStage>(s, "SetStreamDelay").book;
		if (params)
			if (const char* why = DelayParamsError(*params, book.MaxDelay()))
				throw std::runtime_error(std::string("neuralaudio_amd: SetStreamDelay: ") + why
					+ ((params->delaySamples < 1 || params->delaySamples > book.MaxDelay()) ? " (maxDelaySamples = " + std::to_string(book.MaxDelay()) + ")" : std::string()));
		RequireFadeRange(fadeSamples, "SetStreamDelay", "fadeSamples");
		if (book.Fading(s)) throw std::runtime_error("neuralaudio_amd: SetStreamDelay: a delay fade of " + StreamId(s) + " is running");
		book.Set(s, params, fadeSamples);
	}

	bool GpuBatch::GetStreamDelay(int s, DelayParams& out) const
	{
		const DelayStage& st = Require<DelayStage>("GetStreamDelay");
		RequireRow(s, "GetStreamDelay");
		if (!st.book.HasDelay(s)) return false;
		out = st.book.Target(s);
		return true;
	}

	int GpuBatch::StreamDelayFadeRemaining(int s) const
	{
		const DelayStage& st = Require<DelayStage>("StreamDelayFadeRemaining");
		RequireRow(s, "StreamDelayFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// Behind the cabinet stage and in front of the reverb stage, on the stream the models ran on: the table of this call's entries goes up
	// from the next pinned table of the ring (the wait for the launch that read it is bounded), every piece of the call is one launch,
	// and the host mirror moves on by the n samples the caller sees.
	void GpuBatch::DelayStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		tables.Require(book.Rows() <= ringRows && book.Rows() <= stateRows);
		const auto table = tables.Take(batch, book.NumEntries());
		const int count = book.BuildTable(table.host);
		if (count > 0)
		{
			tables.Upload(table, count, launch);
			for (size_t done = 0; done < n; done += (size_t)kDelayPieceSamples)
			{
				const int piece = (int)std::min<size_t>((size_t)kDelayPieceSamples, n - done);
				CheckHip(LaunchDelayStage(DelayLaunch{ table.dev, count, dOut, outStride, (unsigned long long)done, piece, rings, book.RingSamples(),
					reinterpret_cast<DelayFilter*>(state) }, launch), "DelayStageKernel");
			}
			tables.Commit(launch);
		}
		book.Advance(n);
	}

	void GpuBatch::DebugRunDelayStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		DebugRunStage(Require<DelayStage>("DebugRunDelayStage"), "DebugRunDelayStage", hostRows, stride, n);
	}
}
