// output_stage.cpp -- the batch's side of the output stage (gpu_batch.h, output_stage.h): the rules of the calls, the
// tables' lifetime, and the one upload + one launch a processing call with entries enqueues.  The arithmetic and the bookkeeping are
// in output_stage.h.
#include "gpu_batch_internal.h"

namespace na
{
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
		outStage->book.Resize(rows);
		outStage->tables.Ensure(*this, std::max(rows, 16));
	}

	bool GpuBatch::StageHasEntries() const
	{
		return (outStage && outStage->book.HasEntries()) || (cabStage && cabStage->book.HasEntries()) ||
			(gateStage && gateStage->book.HasEntries()) || (eqStage && eqStage->book.HasEntries());
	}

	void GpuBatch::RequireRow(int s, const char* who) const
	{
		if (s < 0 || s >= (int)streams.size() || !streams[(size_t)s].live)
			throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": " + StreamId(s) + " is not a stream of the batch");
	}

	void GpuBatch::SetStreamGain(int s, float gain, int rampSamples)
	{
		CheckUsable();
		OutputStage& st = RequireStage(outStage, "SetStreamGain");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: SetStreamGain: " + StreamId(s) + " is not a live stream of the batch");
		if (!std::isfinite(gain) || gain < 0.0f) throw std::runtime_error("neuralaudio_amd: SetStreamGain: gain must be finite and >= 0");
		if (rampSamples < 0 || rampSamples > kOutStageMaxRamp) throw std::runtime_error("neuralaudio_amd: SetStreamGain: rampSamples must lie in [0, 1 << 20]");
		st.book.SetGain(s, gain, rampSamples);
	}

	float GpuBatch::GetStreamGain(int s) const
	{
		const OutputStage& st = RequireStage(outStage, "GetStreamGain");
		RequireRow(s, "GetStreamGain");
		return st.book.Target(s);
	}

	void GpuBatch::Handover(int from, int to, float quality, int fadeSamples)
	{
		CheckUsable();
		OutputStageBook& book = RequireStage(outStage, "Handover").book;
		if (from == to) throw std::runtime_error("neuralaudio_amd: Handover: from and to are the same stream (" + StreamId(from) + ")");
		if (!IsLive(from)) throw std::runtime_error("neuralaudio_amd: Handover: from (" + StreamId(from) + ") is not a live stream of the batch");
		if (!streams[(size_t)from].pooled)
			throw std::runtime_error("neuralaudio_amd: Handover: from (" + StreamId(from) + ") did not come from ReserveStreams (the hand-over ends in a park)");
		if (!IsParked(to)) throw std::runtime_error("neuralaudio_amd: Handover: to (" + StreamId(to) + ") is not a parked stream of the batch");
		if (fadeSamples < 0 || fadeSamples > kOutStageMaxRamp) throw std::runtime_error("neuralaudio_amd: Handover: fadeSamples must lie in [0, 1 << 20]");
		if (book.FadeOf(from) >= 0) throw std::runtime_error("neuralaudio_amd: Handover: from (" + StreamId(from) + ") is part of a running fade");
		// (`to` is parked, and a parked stream is in no fade: StageLeave ended it)
		// its fade has produced its last sample and the next buffer parks it: a new fade from it would end with that park
		const std::vector<int>& fin = book.Finished();
		if (std::find(fin.begin(), fin.end(), from) != fin.end())
			throw std::runtime_error("neuralaudio_amd: Handover: from (" + StreamId(from) + ") has handed its session over and is parked by the next buffer");
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
		const OutputStage& st = RequireStage(outStage, "HandoverRemaining");
		RequireRow(s, "HandoverRemaining");
		return st.book.FadeRemaining(s);
	}

	// The stream leaves (ParkStream, RemoveStreams): the fade it is part of ends with the next buffer -- the other stream carries on alone
	// at its own gain -- and its own gain is 1 again: a parked stream carries nothing over.
	void GpuBatch::StageLeave(int s)
	{
		GateLeave(s);
		EqLeave(s);
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
		if (st.book.NumEntries() > st.tables.capacity) throw std::runtime_error("neuralaudio_amd: output stage: more entries than the tables hold");
		const auto table = st.tables.Take(*this);
		const int count = st.book.BuildTable(table.host);
		if (count > 0)
		{
			CheckHip(hipMemcpyAsync(table.dev, table.host, (size_t)count * sizeof(OutStageEntry), hipMemcpyHostToDevice, launch), "hipMemcpyAsync (output stage table)");
			CheckHip(LaunchOutputStage(OutStageLaunch{ table.dev, count, dOut, outStride, (unsigned long long)n }, launch), "OutputStageKernel");
			st.tables.Commit(launch);
		}
		st.book.Advance(n);
	}
}
