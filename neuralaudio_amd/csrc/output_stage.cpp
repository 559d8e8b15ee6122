// output_stage.cpp -- the batch's side of the output stage (gpu_batch.h, output_stage.h): the rules of the calls, the
// tables' lifetime, and the one upload + one launch a processing call with entries enqueues.  The arithmetic and the bookkeeping are
// in output_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what every stage shares is in
// gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	void GpuBatch::EnableOutputStage() { EnableStage<OutputStage>(); }

	// set-up side (EnableOutputStage, CreateStreams): every table holds an entry per row -- a stream is part of one entry at most
	void GpuBatch::OutputStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		tables.Ensure(batch, std::max(rows, 16));
	}

	void GpuBatch::RequireRow(int s, const char* who) const
	{
		if (s < 0 || s >= (int)streams.size() || !streams[(size_t)s].live)
			throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": " + StreamId(s) + " is not a stream of the batch");
	}

	void GpuBatch::SetStreamGain(int s, float gain, int rampSamples)
	{
		CheckUsable();
		OutputStage& st = Require<OutputStage>("SetStreamGain");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: SetStreamGain: " + StreamId(s) + " is not a live stream of the batch");
		if (!std::isfinite(gain) || gain < 0.0f) throw std::runtime_error("neuralaudio_amd: SetStreamGain: gain must be finite and >= 0");
		RequireFadeRange(rampSamples, "SetStreamGain", "rampSamples");
		st.book.SetGain(s, gain, rampSamples);
	}

	float GpuBatch::GetStreamGain(int s) const
	{
		const OutputStage& st = Require<OutputStage>("GetStreamGain");
		RequireRow(s, "GetStreamGain");
		return st.book.Target(s);
	}

	void GpuBatch::Handover(int from, int to, float quality, int fadeSamples)
	{
		CheckUsable();
		OutputStageBook& book = Require<OutputStage>("Handover").book;
		if (from == to) throw std::runtime_error("neuralaudio_amd: Handover: from and to are the same stream (" + StreamId(from) + ")");
		if (!IsLive(from)) throw std::runtime_error("neuralaudio_amd: Handover: from (" + StreamId(from) + ") is not a live stream of the batch");
		if (!streams[(size_t)from].pooled)
			throw std::runtime_error("neuralaudio_amd: Handover: from (" + StreamId(from) + ") did not come from ReserveStreams (the hand-over ends in a park)");
		if (!IsParked(to)) throw std::runtime_error("neuralaudio_amd: Handover: to (" + StreamId(to) + ") is not a parked stream of the batch");
		RequireFadeRange(fadeSamples, "Handover", "fadeSamples");
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
		const OutputStage& st = Require<OutputStage>("HandoverRemaining");
		RequireRow(s, "HandoverRemaining");
		return st.book.FadeRemaining(s);
	}

	// The stream leaves (ParkStream, RemoveStreams): the fade it is part of ends with the next buffer -- the other stream carries on alone
	// at its own gain -- and its own gain is 1 again: a parked stream carries nothing over.
	void GpuBatch::OutputStage::Leave(int s)
	{
		if (s >= book.Rows()) return;
		(void)book.EndFadeOf(s);
		book.ResetGain(s);
		std::vector<int>& fin = book.Finished();
		fin.erase(std::remove(fin.begin(), fin.end(), s), fin.end());
	}

	// The fades that produced their last sample in the previous call: their `from` streams are parked now, in front of this call's list
	// uploads, so that this is the first buffer without them.
	void GpuBatch::StageParkFinished()
	{
		std::vector<int>& fin = Require<OutputStage>("StageParkFinished").book.Finished();
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
	void GpuBatch::OutputStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		const auto table = tables.Take(batch, book.NumEntries());
		const int count = book.BuildTable(table.host);
		if (count > 0)
		{
			tables.Upload(table, count, launch);
			CheckHip(LaunchOutputStage(OutStageLaunch{ table.dev, count, dOut, outStride, (unsigned long long)n }, launch), "OutputStageKernel");
			tables.Commit(launch);
		}
		book.Advance(n);
	}
}
