// reverb_stage.cpp -- the batch's side of the reverb stage (gpu_batch.h, reverb_stage.h): the rules of the calls, the
// lifetime of rings, spectra, tables and IRs, the load-side transform of an IR and the one upload + up to four launches per piece a
// processing call with entries enqueues.  The arithmetic's order and the bookkeeping are in reverb_stage.h; the stage's place in the
// chain is GpuBatch::StageId (gpu_batch.h), what every stage shares is in gpu_batch_internal.h.
#include <cmath>

#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::ReverbStage::~ReverbStage()
	{
		for (float* p : { rings, spectra, tails, twiddles })
			if (p) (void)CountedHipFree(p);
		for (int ir = 0; ir < book.IRSlots(); ir++)
			if (book.IsLoaded(ir)) (void)CountedHipFree(const_cast<float*>(book.DataOf(ir)));
	}

	void GpuBatch::EnableReverbStage(int maxTaps)
	{
		CheckUsable();
		if (maxTaps < 1 || maxTaps > kRevMaxTaps) throw std::runtime_error("neuralaudio_amd: EnableReverbStage: maxTaps must lie in [1, 131072]");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!stages[kReverbStage]) stages[kReverbStage].reset(new ReverbStage());
		ReverbStage& st = Require<ReverbStage>("EnableReverbStage");
		if (maxTaps > st.book.MaxTaps())
		{
			if (st.book.HasEntries()) throw std::runtime_error("neuralaudio_amd: EnableReverbStage: a larger maxTaps is refused while a stream has a reverb");
			if (ReverbBook::SlotsFor(maxTaps) != st.book.Slots() && st.spectra)
			{
				// (no stream has a reverb: no history to carry over; the launches that read the old spectra are over before they go)
				Quiesce();
				(void)CountedHipFree(st.spectra);
				st.spectra = nullptr;
				st.spectraRows = 0;
			}
			st.book.Configure(maxTaps);
		}
		if (!st.twiddles)
		{
			CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&st.twiddles), (size_t)kRevPoints * sizeof(float)), "hipMalloc (reverb twiddles)");
			CheckHip(hipMemcpy(st.twiddles, ReverbTwiddles(), (size_t)kRevPoints * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy (reverb twiddles)");
		}
		EnableStage<ReverbStage>();
	}

	// set-up side (EnableReverbStage, CreateStreams): a sample ring, a ring of spectra and the tail blocks per row, tables that hold an
	// entry per row
	void GpuBatch::ReverbStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want);
		if (want > ringRows || want > spectraRows)
		{
			// the rows that exist keep their histories: whatever reads or writes the old blocks is over before they are copied
			if (rings || spectra) batch.Quiesce();
			if (want > ringRows)
			{
				batch.GrowRowBlock(rings, (size_t)kRevRingSamples, ringRows, want, "hipMalloc (reverb rings)", "reverb rings");
				batch.GrowRowBlock(tails, (size_t)kRevTailFloats, ringRows, want, "hipMalloc (reverb tails)", "reverb tails");
				ringRows = want;
			}
			if (want > spectraRows)
			{
				batch.GrowRowBlock(spectra, (size_t)book.Slots() * kRevSpectrumFloats, spectraRows, want, "hipMalloc (reverb spectra)", "reverb spectra");
				spectraRows = want;
			}
		}
	}

	ReverbStageInfo GpuBatch::GetReverbInfo() const
	{
		const ReverbStage& st = Require<ReverbStage>("GetReverbInfo");
		ReverbStageInfo info;
		info.maxTaps = st.book.MaxTaps();
		info.partitionSamples = kRevPartition;
		info.slots = st.book.Slots();
		info.pieceSamples = kRevPieceSamples;
		info.numIRs = st.book.NumIRs();
		info.deviceBytes = (long long)st.ringRows * (kRevRingSamples + kRevTailFloats) * (long long)sizeof(float)
			+ (long long)st.spectraRows * st.book.Slots() * kRevSpectrumFloats * (long long)sizeof(float) + kRevPoints * (long long)sizeof(float) + st.tables.Bytes()
			+ st.irBytes;
		return info;
	}

	// Load side: the taps go up padded with zeros to whole partitions, the stage's own transform makes H_1 .. H_{J-1} of them on the
	// device, and the call waits -- under the wait limit -- until they are there.
	int GpuBatch::LoadReverbIR(const float* taps, int numTaps)
	{
		CheckUsable();
		ReverbStage& st = Require<ReverbStage>("LoadReverbIR");
		if (!taps || numTaps < 1 || numTaps > st.book.MaxTaps())
			throw std::runtime_error("neuralaudio_amd: LoadReverbIR: numTaps must lie in [1, maxTaps] (maxTaps = " + std::to_string(st.book.MaxTaps()) + ")");
		for (int k = 0; k < numTaps; k++)
			if (!std::isfinite(taps[k])) throw std::runtime_error("neuralaudio_amd: LoadReverbIR: the taps must be finite (tap " + std::to_string(k) + " is not)");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		const int J = RevPartitions(numTaps);
		std::vector<float> padded((size_t)J * kRevPartition, 0.0f);
		std::copy(taps, taps + numTaps, padded.begin());
		const size_t irBytes = RevIRFloats(numTaps) * sizeof(float);
		float *dTaps = nullptr, *dIR = nullptr;
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dTaps), padded.size() * sizeof(float)), "hipMalloc (reverb IR taps)");
		hipError_t e = CountedHipMalloc(reinterpret_cast<void**>(&dIR), irBytes);
		if (e == hipSuccess) e = hipMemcpyAsync(dTaps, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice, stream);
		if (e == hipSuccess) e = hipMemcpyAsync(dIR, dTaps, (size_t)kRevPartition * sizeof(float), hipMemcpyDeviceToDevice, stream);
		if (e == hipSuccess) e = LaunchReverbIR(RevIRLaunch{ dTaps, dIR, J, st.twiddles }, stream);
		try
		{
			CheckHip(e, "LoadReverbIR");
			WaitStreamBounded(stream, "hipStreamSynchronize"); // (`padded` is pageable: the copy has read it by now in any case)
		}
		catch (...)
		{
			if (!IsBroken())
			{
				(void)CountedHipFree(dTaps);
				if (dIR) (void)CountedHipFree(dIR);
			}
			throw;
		}
		(void)CountedHipFree(dTaps);
		st.irBytes += (long long)irBytes;
		return st.book.AddIR(dIR, numTaps);
	}

	void GpuBatch::UnloadReverbIR(int ir)
	{
		CheckUsable();
		ReverbStage& st = Require<ReverbStage>("UnloadReverbIR");
		if (!st.book.IsLoaded(ir)) throw std::runtime_error("neuralaudio_amd: UnloadReverbIR: IR " + std::to_string(ir) + " is not loaded");
		if (st.book.Users(ir) > 0) throw std::runtime_error("neuralaudio_amd: UnloadReverbIR: IR " + std::to_string(ir) + " is in use (a stream has it or fades from it)");
		Quiesce(); // (the last launch that read it may still run)
		st.irBytes -= (long long)(RevIRFloats(st.book.Taps(ir)) * sizeof(float));
		(void)CountedHipFree(const_cast<float*>(st.book.RemoveIR(ir)));
	}

	void GpuBatch::SetStreamReverb(int s, int ir, float wet, float dry, int fadeSamples)
	{
		ReverbBook& book = SettableStage<ReverbStage>(s, "SetStreamReverb").book;
		if (ir != kRevDry && !book.IsLoaded(ir)) throw std::runtime_error("neuralaudio_amd: SetStreamReverb: IR " + std::to_string(ir) + " is not loaded");
		if (ir != kRevDry && (!std::isfinite(wet) || !std::isfinite(dry))) throw std::runtime_error("neuralaudio_amd: SetStreamReverb: wet and dry must be finite");
		RequireFadeRange(fadeSamples, "SetStreamReverb", "fadeSamples");
		if (book.Fading(s)) throw std::runtime_error("neuralaudio_amd: SetStreamReverb: a reverb fade of " + StreamId(s) + " is running");
		book.Set(s, ir, wet, dry, fadeSamples);
	}

	int GpuBatch::GetStreamReverb(int s, float* wet, float* dry) const
	{
		const ReverbStage& st = Require<ReverbStage>("GetStreamReverb");
		RequireRow(s, "GetStreamReverb");
		if (wet) *wet = st.book.TargetWet(s);
		if (dry) *dry = st.book.TargetDry(s);
		return st.book.Target(s);
	}

	int GpuBatch::StreamReverbFadeRemaining(int s) const
	{
		const ReverbStage& st = Require<ReverbStage>("StreamReverbFadeRemaining");
		RequireRow(s, "StreamReverbFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// Behind the cabinet stage and in front of the output stage, on the stream the models ran on: the table of this call's entries goes
	// up from the next pinned table of the ring (the wait for the launch that read it is bounded), every piece of the call is the append
	// and apply launches and -- where a block is completed / a tail is needed -- the spectrum and tail launches between them, and the
	// host mirror moves on by the n samples the caller sees.
	void GpuBatch::ReverbStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		tables.Require(book.Rows() <= ringRows && book.Rows() <= spectraRows);
		const auto table = tables.Take(batch, book.NumEntries());
		const int count = book.BuildTable(table.host);
		if (count > 0)
		{
			tables.Upload(table, count, launch);
			for (size_t done = 0; done < n; done += (size_t)kRevPieceSamples)
			{
				const int piece = (int)std::min<size_t>((size_t)kRevPieceSamples, n - done);
				const ReverbBook::PieceNeeds needs = book.NeedsOf(done, piece);
				CheckHip(LaunchReverbStage(RevLaunch{ table.dev, count, dOut, outStride, (unsigned long long)done, piece, twiddles, rings, spectra, tails, book.Slots(),
					needs.spectra, needs.tails }, launch), "ReverbStageKernel");
			}
			tables.Commit(launch);
		}
		book.Advance(n);
	}

	void GpuBatch::DebugRunReverbStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		DebugRunStage(Require<ReverbStage>("DebugRunReverbStage"), "DebugRunReverbStage", hostRows, stride, n);
	}
}
