// cabinet_stage.cpp -- the batch's side of the cabinet stage (gpu_batch.h, cabinet_stage.h): the rules of the calls, the
// lifetime of rings, tables and IRs, and the one upload + two launches per piece a processing call with entries enqueues.  The
// arithmetic's order and the bookkeeping are in cabinet_stage.h.
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
		if (!cabStage) cabStage.reset(new CabinetStage());
		CabinetStage& st = *cabStage;
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
		EnsureCabinetRows((int)streams.size());
		EnsurePoolPipeline(); // (an entry moves Submit's buffers onto the slots' own streams or the copy streams: they exist from here on)
	}

	// set-up side (EnableCabinetStage, CreateStreams): a ring per row, tables that hold an entry per row
	void GpuBatch::EnsureCabinetRows(int rows)
	{
		CabinetStage& st = *cabStage;
		st.book.Resize(rows);
		const int want = std::max(rows, 16);
		st.tables.Ensure(*this, want);
		if (want > st.ringRows)
		{
			// the rows that exist keep their histories: whatever reads or writes the old rings is over before they are copied
			if (st.rings) Quiesce();
			GrowRowBlock(st.rings, (size_t)st.book.RingSamples(), st.ringRows, want, "hipMalloc (cabinet rings)", "cabinet rings");
			st.ringRows = want;
		}
	}

	CabinetStageInfo GpuBatch::GetCabinetInfo() const
	{
		const CabinetStage& st = RequireStage(cabStage, "GetCabinetInfo");
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
		CabinetStage& st = RequireStage(cabStage, "LoadIR");
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
		CabinetStage& st = RequireStage(cabStage, "UnloadIR");
		if (!st.book.IsLoaded(ir)) throw std::runtime_error("neuralaudio_amd: UnloadIR: IR " + std::to_string(ir) + " is not loaded");
		if (st.book.Users(ir) > 0) throw std::runtime_error("neuralaudio_amd: UnloadIR: IR " + std::to_string(ir) + " is in use (a stream has it or fades from it)");
		Quiesce(); // (the last launch that read it may still run)
		st.tapBytes -= (long long)((size_t)(st.book.Taps(ir) + 3) / 4 * 4 * sizeof(float));
		(void)CountedHipFree(const_cast<float*>(st.book.RemoveIR(ir)));
	}

	void GpuBatch::SetStreamIR(int s, int ir, int fadeSamples)
	{
		CheckUsable();
		CabinetBook& book = RequireStage(cabStage, "SetStreamIR").book;
		if (IsParked(s)) throw std::runtime_error("neuralaudio_amd: SetStreamIR: " + StreamId(s) + " is parked");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: SetStreamIR: " + StreamId(s) + " is not a live stream of the batch");
		if (ir != kCabDry && !book.IsLoaded(ir)) throw std::runtime_error("neuralaudio_amd: SetStreamIR: IR " + std::to_string(ir) + " is not loaded");
		if (fadeSamples < 0 || fadeSamples > kOutStageMaxRamp) throw std::runtime_error("neuralaudio_amd: SetStreamIR: fadeSamples must lie in [0, 1 << 20]");
		if (book.Fading(s)) throw std::runtime_error("neuralaudio_amd: SetStreamIR: an IR fade of " + StreamId(s) + " is running");
		book.SetIR(s, ir, fadeSamples);
	}

	int GpuBatch::GetStreamIR(int s) const
	{
		const CabinetStage& st = RequireStage(cabStage, "GetStreamIR");
		RequireRow(s, "GetStreamIR");
		return st.book.Target(s);
	}

	int GpuBatch::StreamIRFadeRemaining(int s) const
	{
		const CabinetStage& st = RequireStage(cabStage, "StreamIRFadeRemaining");
		RequireRow(s, "StreamIRFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// The stream leaves (ParkStream, RemoveStreams): dry at once, its history dropped -- a parked stream carries nothing over
	void GpuBatch::CabinetLeave(int s)
	{
		if (!cabStage || s >= cabStage->book.Rows()) return;
		cabStage->book.Leave(s);
	}

	// Behind the model launches of the call and in front of the output stage, on the stream they ran on: the table of this call's entries
	// goes up from the next pinned table of the ring (the wait for the launch that read it is bounded), every piece of the call is two
	// launches, and the host mirror moves on by the n samples the caller sees.
	void GpuBatch::RunCabinetStage(hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		CabinetStage& st = *cabStage;
		if (st.book.NumEntries() > st.tables.capacity || st.book.Rows() > st.ringRows) throw std::runtime_error("neuralaudio_amd: cabinet stage: more entries than the tables hold");
		const auto table = st.tables.Take(*this);
		const int count = st.book.BuildTable(table.host);
		if (count > 0)
		{
			CheckHip(hipMemcpyAsync(table.dev, table.host, (size_t)count * sizeof(CabEntry), hipMemcpyHostToDevice, launch), "hipMemcpyAsync (cabinet stage table)");
			for (size_t done = 0; done < n; done += (size_t)kCabPieceSamples)
			{
				const int piece = (int)std::min<size_t>((size_t)kCabPieceSamples, n - done);
				CheckHip(LaunchCabinetStage(CabLaunch{ table.dev, count, dOut, outStride, (unsigned long long)done, piece, st.rings, st.book.RingSamples() }, launch),
					"CabinetStageKernel");
			}
			st.tables.Commit(launch);
		}
		st.book.Advance(n);
	}

	// test hook (NA_DebugRunCabinetStage): what a processing call of n samples runs for the stage, on host rows in place of model outputs
	void GpuBatch::DebugRunCabinetStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		const CabinetStage& st = RequireStage(cabStage, "DebugRunCabinetStage");
		if (!hostRows || n == 0 || stride < (long)n || streams.empty()) throw std::runtime_error("neuralaudio_amd: DebugRunCabinetStage: bad argument");
		Quiesce();
		if (!st.book.HasEntries()) return;
		const size_t floats = (size_t)streams.size() * (size_t)stride;
		float* dRows = nullptr;
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dRows), floats * sizeof(float)), "hipMalloc");
		try
		{
			CheckHip(hipMemcpyAsync(dRows, hostRows, floats * sizeof(float), hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
			RunCabinetStage(stream, dRows, n, stride);
			CheckHip(hipMemcpyAsync(hostRows, dRows, floats * sizeof(float), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
			WaitStreamBounded(stream, "hipStreamSynchronize");
		}
		catch (...)
		{
			if (!broken) (void)CountedHipFree(dRows);
			throw;
		}
		(void)CountedHipFree(dRows);
	}
}
