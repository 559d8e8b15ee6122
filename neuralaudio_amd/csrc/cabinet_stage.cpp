// cabinet_stage.cpp -- the batch's side of the cabinet stage (gpu_batch.h, cabinet_stage.h): the rules of the calls, the
// lifetime of rings, tables and IRs, and the one upload + two launches per piece a processing call with entries enqueues.  The
// arithmetic's order and the bookkeeping are in cabinet_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what
// every stage shares is in gpu_batch_internal.h.
#include <cmath>

#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::CabinetStage::~CabinetStage()
	{
		if (rings) (void)CountedHipFree(rings);
		for (int ir = 0; ir < book.IRSlots(); ir++)
			if (book.IsLoaded(ir)) (void)CountedHipFree(const_cast<float*>(book.TapsOf(ir)));
	}

	void GpuBatch::EnableCabinetStage(int maxTaps)
	{
		CheckUsable();
		if (maxTaps < 1 || maxTaps > kCabMaxTaps) throw std::runtime_error("neuralaudio_amd: EnableCabinetStage: maxTaps must lie in [1, 8192]");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!stages[kCabinetStage]) stages[kCabinetStage].reset(new CabinetStage());
		CabinetStage& st = Require<CabinetStage>("EnableCabinetStage");
		if (maxTaps > st.book.MaxTaps())
		{
			if (st.book.HasEntries()) throw std::runtime_error("neuralaudio_amd: EnableCabinetStage: a larger maxTaps is refused while a stream has an IR");
			if (CabinetBook::RingFor(maxTaps) != st.book.RingSamples() && st.rings)
			{
				// (no stream has an IR: no history to carry over; the launches that read the old rings are over before they go)
				Quiesce();
				(void)CountedHipFree(st.rings);
				st.rings = nullptr;
				st.ringRows = 0;
			}
			st.book.Configure(maxTaps);
		}
		EnableStage<CabinetStage>();
	}

	// set-up side (EnableCabinetStage, CreateStreams): a ring per row, tables that hold an entry per row
	void GpuBatch::CabinetStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want);
		if (want > ringRows)
		{
			// the rows that exist keep their histories: whatever reads or writes the old rings is over before they are copied
			if (rings) batch.Quiesce();
			batch.GrowRowBlock(rings, (size_t)book.RingSamples(), ringRows, want, "hipMalloc (cabinet rings)", "cabinet rings");
			ringRows = want;
		}
	}

	CabinetStageInfo GpuBatch::GetCabinetInfo() const
	{
		const CabinetStage& st = Require<CabinetStage>("GetCabinetInfo");
		CabinetStageInfo info;
		info.maxTaps = st.book.MaxTaps();
		info.ringSamples = st.book.RingSamples();
		info.pieceSamples = kCabPieceSamples;
		info.numIRs = st.book.NumIRs();
		info.deviceBytes = (long long)st.ringRows * st.book.RingSamples() * (long long)sizeof(float) + st.tables.Bytes() + st.tapBytes;
		return info;
	}

	int GpuBatch::LoadIR(const float* taps, int numTaps)
	{
		CheckUsable();
		CabinetStage& st = Require<CabinetStage>("LoadIR");
		if (!taps || numTaps < 1 || numTaps > st.book.MaxTaps())
			throw std::runtime_error("neuralaudio_amd: LoadIR: numTaps must lie in [1, maxTaps] (maxTaps = " + std::to_string(st.book.MaxTaps()) + ")");
		for (int k = 0; k < numTaps; k++)
			if (!std::isfinite(taps[k])) throw std::runtime_error("neuralaudio_amd: LoadIR: the taps must be finite (tap " + std::to_string(k) + " is not)");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		// padded with zeros to a multiple of four: the kernel's last quad of taps
		std::vector<float> padded((size_t)(numTaps + 3) / 4 * 4, 0.0f);
		std::copy(taps, taps + numTaps, padded.begin());
		float* dTaps = nullptr;
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dTaps), padded.size() * sizeof(float)), "hipMalloc (IR)");
		const hipError_t e = hipMemcpy(dTaps, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice);
		if (e != hipSuccess)
		{
			(void)CountedHipFree(dTaps);
			CheckHip(e, "hipMemcpy (IR)");
		}
		st.tapBytes += (long long)(padded.size() * sizeof(float));
		return st.book.AddIR(dTaps, numTaps);
	}

	void GpuBatch::UnloadIR(int ir)
	{
		CheckUsable();
		CabinetStage& st = Require<CabinetStage>("UnloadIR");
		if (!st.book.IsLoaded(ir)) throw std::runtime_error("neuralaudio_amd: UnloadIR: IR " + std::to_string(ir) + " is not loaded");
		if (st.book.Users(ir) > 0) throw std::runtime_error("neuralaudio_amd: UnloadIR: IR " + std::to_string(ir) + " is in use (a stream has it or fades from it)");
		Quiesce(); // (the last launch that read it may still run)
		st.tapBytes -= (long long)((size_t)(st.book.Taps(ir) + 3) / 4 * 4 * sizeof(float));
		(void)CountedHipFree(const_cast<float*>(st.book.RemoveIR(ir)));
	}

	void GpuBatch::SetStreamIR(int s, int ir, int fadeSamples)
	{
		CabinetBook& book = SettableStage<CabinetStage>(s, "SetStreamIR").book;
		if (ir != kCabDry && !book.IsLoaded(ir)) throw std::runtime_error("neuralaudio_amd: SetStreamIR: IR " + std::to_string(ir) + " is not loaded");
		RequireFadeRange(fadeSamples, "SetStreamIR", "fadeSamples");
		if (book.Fading(s)) throw std::runtime_error("neuralaudio_amd: SetStreamIR: an IR fade of " + StreamId(s) + " is running");
		book.SetIR(s, ir, fadeSamples);
	}

	int GpuBatch::GetStreamIR(int s) const
	{
		const CabinetStage& st = Require<CabinetStage>("GetStreamIR");
		RequireRow(s, "GetStreamIR");
		return st.book.Target(s);
	}

	int GpuBatch::StreamIRFadeRemaining(int s) const
	{
		const CabinetStage& st = Require<CabinetStage>("StreamIRFadeRemaining");
		RequireRow(s, "StreamIRFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// Behind the model launches of the call and in front of the output stage, on the stream they ran on: the table of this call's entries
	// goes up from the next pinned table of the ring (the wait for the launch that read it is bounded), every piece of the call is two
	// launches, and the host mirror moves on by the n samples the caller sees.
	void GpuBatch::CabinetStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		tables.Require(book.Rows() <= ringRows);
		const auto table = tables.Take(batch, book.NumEntries());
		const int count = book.BuildTable(table.host);
		if (count > 0)
		{
			tables.Upload(table, count, launch);
			for (size_t done = 0; done < n; done += (size_t)kCabPieceSamples)
			{
				const int piece = (int)std::min<size_t>((size_t)kCabPieceSamples, n - done);
				CheckHip(LaunchCabinetStage(CabLaunch{ table.dev, count, dOut, outStride, (unsigned long long)done, piece, rings, book.RingSamples() }, launch),
					"CabinetStageKernel");
			}
			tables.Commit(launch);
		}
		book.Advance(n);
	}

	void GpuBatch::DebugRunCabinetStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		DebugRunStage(Require<CabinetStage>("DebugRunCabinetStage"), "DebugRunCabinetStage", hostRows, stride, n);
	}
}
