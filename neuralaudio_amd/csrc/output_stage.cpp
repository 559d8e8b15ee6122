// output_stage.cpp -- the batch's side of the output stage (gpu_batch.h, output_stage.h): the rules of the calls, the
// tables' lifetime, and the one upload + one launch a processing call with entries enqueues.  The arithmetic and the bookkeeping are
// in output_stage.h.
#include "gpu_batch_internal.h"

namespace na
{
	namespace
	{
		std::string Id(int s) { return "stream " + std::to_string(s); }
	}

	void GpuBatch::EnableOutputStage()
	{
		CheckUsable();
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!outStage) outStage.reset(new OutputStage());
		EnsureStageRows((int)streams.size());
		EnsurePoolPipeline(); // (an entry moves Submit's buffers onto the slots' own streams or the copy streams: they exist from here on)
	}

	// set-up side (EnableOutputStage, CreateStreams): every table holds an entry per row -- a stream is part of one entry at most
	void GpuBatch::EnsureStageRows(int rows)
	{
		OutputStage& st = *outStage;
		st.book.Resize(rows);
		for (int i = 0; i < OutputStage::kTables; i++)
			if (!st.done[i]) CheckHip(CountedHipEventCreateWithFlags(&st.done[i], hipEventDisableTiming), "hipEventCreate");
		const int want = std::max(rows, 16);
		if (want <= st.capacity) return;
		for (int i = 0; i < OutputStage::kTables; i++)
		{
			// (the launch that reads the old table is over before it goes)
			if (st.used[i]) WaitEventBounded(st.done[i], "output stage: table in flight");
			st.used[i] = false;
			if (st.host[i]) (void)CountedHipHostFree(st.host[i]);
			if (st.dev[i]) (void)CountedHipFree(st.dev[i]);
			st.host[i] = st.dev[i] = nullptr;
		}
		st.capacity = 0;
		for (int i = 0; i < OutputStage::kTables; i++)
		{
			CheckHip(CountedHipHostMalloc(reinterpret_cast<void**>(&st.host[i]), (size_t)want * sizeof(OutStageEntry), hipHostMallocDefault), "hipHostMalloc");
			CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&st.dev[i]), (size_t)want * sizeof(OutStageEntry)), "hipMalloc");
		}
		st.capacity = want;
	}

	bool GpuBatch::StageHasEntries() const { return (outStage && outStage->book.HasEntries()) || (cabStage && cabStage->book.HasEntries()); }

	void GpuBatch::SetStreamGain(int s, float gain, int rampSamples)
	{
		CheckUsable();
		if (!outStage) throw std::runtime_error("neuralaudio_amd: SetStreamGain: output stage not enabled (NA_BatchEnableOutputStage)");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: SetStreamGain: " + Id(s) + " is not a live stream of the batch");
		if (!std::isfinite(gain) || gain < 0.0f) throw std::runtime_error("neuralaudio_amd: SetStreamGain: gain must be finite and >= 0");
		if (rampSamples < 0 || rampSamples > kOutStageMaxRamp) throw std::runtime_error("neuralaudio_amd: SetStreamGain: rampSamples must lie in [0, 1 << 20]");
		outStage->book.SetGain(s, gain, rampSamples);
	}

	float GpuBatch::GetStreamGain(int s) const
	{
		if (!outStage) throw std::runtime_error("neuralaudio_amd: GetStreamGain: output stage not enabled (NA_BatchEnableOutputStage)");
		if (s < 0 || s >= (int)streams.size() || !streams[(size_t)s].live) throw std::runtime_error("neuralaudio_amd: GetStreamGain: " + Id(s) + " is not a stream of the batch");
		return outStage->book.Target(s);
	}

	void GpuBatch::Handover(int from, int to, float quality, int fadeSamples)
	{
		CheckUsable();
		if (!outStage) throw std::runtime_error("neuralaudio_amd: Handover: output stage not enabled (NA_BatchEnableOutputStage)");
		if (from == to) throw std::runtime_error("neuralaudio_amd: Handover: from and to are the same stream (" + Id(from) + ")");
		if (!IsLive(from)) throw std::runtime_error("neuralaudio_amd: Handover: from (" + Id(from) + ") is not a live stream of the batch");
		if (!streams[(size_t)from].pooled)
			throw std::runtime_error("neuralaudio_amd: Handover: from (" + Id(from) + ") did not come from ReserveStreams (the hand-over ends in a park)");
		if (!IsParked(to)) throw std::runtime_error("neuralaudio_amd: Handover: to (" + Id(to) + ") is not a parked stream of the batch");
		if (fadeSamples < 0 || fadeSamples > kOutStageMaxRamp) throw std::runtime_error("neuralaudio_amd: Handover: fadeSamples must lie in [0, 1 << 20]");
		OutputStageBook& book = outStage->book;
		if (book.FadeOf(from) >= 0) throw std::runtime_error("neuralaudio_amd: Handover: from (" + Id(from) + ") is part of a running fade");
		// (`to` is parked, and a parked stream is in no fade: StageLeave ended it)
		// its fade has produced its last sample and the next buffer parks it: a new fade from it would end with that park
		const std::vector<int>& fin = book.Finished();
		if (std::find(fin.begin(), fin.end(), from) != fin.end())
			throw std::runtime_error("neuralaudio_amd: Handover: from (" + Id(from) + ") has handed its session over and is parked by the next buffer");
		ActivateStream(to, quality);
		if (fadeSamples == 0)
		{
			ParkStream(from); // w = 1 at once: activate + park with nothing in between
			return;
		}
		if (!book.BeginFade(from, to, fadeSamples)) throw std::runtime_error("neuralaudio_amd: Handover: no free fade slot");
	}

	int GpuBatch::HandoverRemaining(int s) const
	{
		if (!outStage) throw std::runtime_error("neuralaudio_amd: HandoverRemaining: output stage not enabled (NA_BatchEnableOutputStage)");
		if (s < 0 || s >= (int)streams.size() || !streams[(size_t)s].live) throw std::runtime_error("neuralaudio_amd: HandoverRemaining: " + Id(s) + " is not a stream of the batch");
		return outStage->book.FadeRemaining(s);
	}

	// The stream leaves (ParkStream, RemoveStreams): the fade it is part of ends with the next buffer -- the other stream carries on alone
	// at its own gain -- and its own gain is 1 again: a parked stream carries nothing over.
	void GpuBatch::StageLeave(int s)
	{
		CabinetLeave(s);
		if (!outStage || s >= outStage->book.Rows()) return;
		OutputStageBook& book = outStage->book;
		(void)book.EndFadeOf(s);
		book.ResetGain(s);
		std::vector<int>& fin = book.Finished();
		fin.erase(std::remove(fin.begin(), fin.end(), s), fin.end());
	}

	// The fades that produced their last sample in the previous call: their `from` streams are parked now, in front of this call's list
	// uploads, so that this is the first buffer without them.
	void GpuBatch::StageParkFinished()
	{
		std::vector<int>& fin = outStage->book.Finished();
		while (!fin.empty())
		{
			const int s = fin.back();
			fin.pop_back();
			if (IsLive(s) && streams[(size_t)s].pooled) ParkStream(s);
		}
	}

	// Behind the model launches of the call, on the stream they ran on (or joined into): the table of this call's entries goes up from
	// the next pinned table of the ring -- one more than buffers can be in flight, so the launch that read it is over; the wait is bounded -- the
	// stage launches, and the host mirror moves on by the n samples the caller sees.
	void GpuBatch::RunOutputStage(hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		OutputStage& st = *outStage;
		if (st.book.NumEntries() > st.capacity) throw std::runtime_error("neuralaudio_amd: output stage: more entries than the tables hold");
		const int b = st.next;
		if (st.used[b]) WaitEventBounded(st.done[b], "output stage: table in flight");
		const int count = st.book.BuildTable(st.host[b]);
		if (count > 0)
		{
			CheckHip(hipMemcpyAsync(st.dev[b], st.host[b], (size_t)count * sizeof(OutStageEntry), hipMemcpyHostToDevice, launch), "hipMemcpyAsync (output stage table)");
			CheckHip(LaunchOutputStage(OutStageLaunch{ st.dev[b], count, dOut, outStride, (unsigned long long)n }, launch), "OutputStageKernel");
			CheckHip(hipEventRecord(st.done[b], launch), "hipEventRecord");
			st.used[b] = true;
			st.next = (b + 1) % OutputStage::kTables;
		}
		st.book.Advance(n);
	}
}
