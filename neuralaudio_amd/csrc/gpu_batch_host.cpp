// gpu_batch_host.cpp -- the host-buffer entry points of GpuBatch (gpu_batch.h): the blocking call (ProcessHost), registered host blocks, and
// the pipelined Submit / Collect interface with its pinned slots.  Reference counterpart: the caller's float* buffers of
// NeuralModel::Process (NeuralAudio/NeuralModel.h:127) -- here [streams][n] arrays in host memory.
#include "gpu_batch_internal.h"

#include <mutex>

namespace na
{
	// every buffer still in flight on a slot stream (pipelined interface) is done after this
	void GpuBatch::DrainPipeline()
	{
		DrainResident();
		for (PipeSlot& p : pipe)
			if (p.own) WaitStreamBounded(p.own, "hipStreamSynchronize");
		WaitChains();
		inFlight->halfChainsUsed = false; // (the next half-batch launches wait for the batch stream first: LaunchHalves)
	}

	// the address under which the device reads a pinned block itself; nullptr: it cannot (not seen on MI355X)
	static float* DeviceAlias(float* pinned)
	{
		float* d = nullptr;
		return hipHostGetDevicePointer(reinterpret_cast<void**>(&d), pinned, 0) == hipSuccess ? d : nullptr;
	}

	void GpuBatch::EnsureStaging(size_t floats)
	{
		if (floats <= stageFloats) return;
		if (hostStage) (void)CountedHipHostFree(hostStage);
		if (devStage) (void)CountedHipFree(devStage);
		hostStage = nullptr;
		devStage = nullptr;
		stageFloats = 0;
		CheckHip(CountedHipHostMalloc(reinterpret_cast<void**>(&hostStage), floats * sizeof(float), hipHostMallocDefault), "hipHostMalloc");
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&devStage), floats * sizeof(float)), "hipMalloc");
		stageFloats = floats;
	}

	// Direct mode (the default; NA_HOST_DIRECT=0 selects the copy engines): the kernels read the block straight from the pinned host buffer
	// and write their output straight into it (every kernel touches `in` once in its prologue and `out` once in its head), so a buffer
	// is ONE launch instead of copy + launch + copy.  The 2 x 512 KB of a 1024 x 128 block still cross PCIe, inside the kernel, but the
	// two asynchronous copies (each ~10 us of latency before its first byte moves) and the waits between them are gone.  Measured on
	// MI355X with this round's kernels (tools/HostPipeBench, 1024 streams x 128 frames; round 2 had it the other way round for the
	// pipelined path, 66.8 vs 61.9 us, and kept the copies):
	//   A1 Standard  Submit..Collect in place 91.8 -> 59.4 us (p50), pipelined 52.9 -> 51.4 us per buffer;  64 streams: 44.9 -> 28.9 us
	//   Nano / Feather / LSTM 1x16 / 2x8      75.8 / 74.6 / 69.4 / 71.2 -> 54.0 / 52.4 / 49.9 / 50.5 us;  A2 96.9 -> 68.4;  4096 Standard 262 -> 180
	bool HostDirect()
	{
		return Tuning::Get().hostDirect;
	}

	// ---- registered host blocks ----
	namespace
	{
		struct HostBlock
		{
			char* host;
			char* dev;
			size_t bytes;
		};
		std::mutex gHostBlocksMutex;
		std::vector<HostBlock> gHostBlocks;
	}
	bool RegisterHostBuffer(void* p, size_t bytes, std::string& error)
	{
		if (!p || bytes == 0) { error = "neuralaudio_amd: RegisterHostBuffer with an empty block"; return false; }
		hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped);
		if (e != hipSuccess) { error = std::string("neuralaudio_amd: hipHostRegister: ") + hipGetErrorString(e); return false; }
		void* d = nullptr;
		e = hipHostGetDevicePointer(&d, p, 0);
		if (e != hipSuccess || !d)
		{
			(void)hipHostUnregister(p);
			error = std::string("neuralaudio_amd: hipHostGetDevicePointer: ") + hipGetErrorString(e);
			return false;
		}
		std::lock_guard<std::mutex> lock(gHostBlocksMutex);
		gHostBlocks.push_back({ static_cast<char*>(p), static_cast<char*>(d), bytes });
		return true;
	}
	bool UnregisterHostBuffer(void* p)
	{
		std::lock_guard<std::mutex> lock(gHostBlocksMutex);
		for (size_t i = 0; i < gHostBlocks.size(); i++)
		{
			if (gHostBlocks[i].host != p) continue;
			gHostBlocks.erase(gHostBlocks.begin() + (long)i);
			return hipHostUnregister(p) == hipSuccess;
		}
		return false;
	}
	void* RegisteredDevicePointer(const void* p, size_t bytes)
	{
		const char* c = static_cast<const char*>(p);
		std::lock_guard<std::mutex> lock(gHostBlocksMutex);
		for (const HostBlock& b : gHostBlocks)
			if (c >= b.host && c + bytes <= b.host + b.bytes) return b.dev + (c - b.host);
		return nullptr;
	}

	// (Splitting the buffer into chunks so that host copies overlap the DMA was measured and dropped: every extra asynchronous copy /
	// event costs more than it hides -- 1024 x 128 frames: 114 us per call as one piece, 134 / 186 / 282 us in 2 / 4 / 8 chunks.)
	void GpuBatch::ProcessHost(const float* in, float* out, size_t n)
	{
		CheckUsable();
		if (n == 0 || streams.empty()) return;
		CheckHip(hipSetDevice(device), "hipSetDevice");
		FlushRearms();
		const size_t total = streams.size() * n;
		BlockingFacts facts = {};
		facts.hostDirect = HostDirect();
		facts.stageEntries = StageHasEntries();
		float *dIn = nullptr, *dOut = nullptr, *dStage = nullptr;
		if (facts.hostDirect)
		{
			dIn = static_cast<float*>(RegisteredDevicePointer(in, total * sizeof(float)));
			dOut = static_cast<float*>(RegisteredDevicePointer(out, total * sizeof(float)));
			facts.bothRegistered = dIn && dOut;
		}
		if (!BlockingRunsOnCallersBlocks(facts))
		{
			EnsureStaging(total);
			if (DirectRows(facts.hostDirect, facts.stageEntries)) dStage = DeviceAlias(hostStage);
			facts.pinnedAddressable = dStage != nullptr;
		}
		const bool halvesPrepared = BlockingTriesHalves(facts) && PrepareHalves(n);
		facts.rowRangesOnly = halvesPrepared && halfLists->RowRangesOnly();
		const HostRoute route = BlockingRouteFor(facts, halvesPrepared);
		lastRoute = (int)route;
		switch (route)
		{
		case HostRoute::RegisteredInPlace:
			// the kernels run on the caller's blocks as they are (no staging copies: 81 -> ~62 us for 1024 x 128)
			ProcessDeviceOrdered(dIn, dOut, n, (long)n, (long)n);
			WaitStreamBounded(stream, "hipStreamSynchronize");
			break;
		case HostRoute::StagedHalves:
			// The blocking call in two halves: the rows of the first half are staged and launched, the second half is staged while the
			// first runs, and the first half's result is copied out while the second still runs -- the two 512 KB host copies of a
			// 1024 x 128 buffer (2 x 10 us) hide behind the kernels: p50 75-77 -> 60 us.
			BeginHalves();
			for (int h = 0; h < numChains; h++)
			{
				for (const WnFrameGroup& g : halfLists->part[h])
					memcpy(hostStage + (size_t)g.row0 * n, in + (size_t)g.row0 * n, (size_t)g.numStreams * n * sizeof(float));
				LaunchChain(h, dStage, dStage, n, (long)n, (long)n, true);
			}
			for (int h = 0; h < numChains; h++)
			{
				WaitStreamBounded(halfStream[h], "hipStreamSynchronize");
				for (const WnFrameGroup& g : halfLists->part[h])
					memcpy(out + (size_t)g.row0 * n, hostStage + (size_t)g.row0 * n, (size_t)g.numStreams * n * sizeof(float));
			}
			inFlight->halfChainsUsed = false; // (both chains are idle again)
			break;
		case HostRoute::StagedInPlace:
		case HostRoute::StagedCopies:
			memcpy(hostStage, in, total * sizeof(float));
			if (route == HostRoute::StagedInPlace)
				ProcessDeviceOrdered(dStage, dStage, n, (long)n, (long)n);
			else
			{
				// (the knob is off, a stage has entries, or -- not seen on MI355X -- the device cannot address the pinned block)
				CheckHip(hipMemcpyAsync(devStage, hostStage, total * sizeof(float), hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
				ProcessDeviceOrdered(devStage, devStage, n, (long)n, (long)n);
				CheckHip(hipMemcpyAsync(hostStage, devStage, total * sizeof(float), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
			}
			JoinHalves();
			WaitStreamBounded(stream, "hipStreamSynchronize");
			memcpy(out, hostStage, total * sizeof(float));
			break;
		default:
			throw std::logic_error("neuralaudio_amd: internal: ProcessHost route");
		}
		ZeroRetiredRows(out, n, streams.size());
	}

	void GpuBatch::ProcessHostToDevice(const float* in, float* dOut, size_t n, long outStride)
	{
		CheckUsable();
		if (n == 0 || streams.empty()) return;
		CheckHip(hipSetDevice(device), "hipSetDevice");
		const size_t total = streams.size() * n;
		// the previous call's kernels may still be reading the pinned block
		WaitStreamBounded(stream, "hipStreamSynchronize");
		FlushRearms();
		EnsureStaging(total);
		memcpy(hostStage, in, total * sizeof(float));
		ToDeviceFacts facts = {};
		facts.hostDirect = HostDirect();
		float* const dStage = facts.hostDirect ? DeviceAlias(hostStage) : nullptr;
		facts.pinnedAddressable = dStage != nullptr;
		const HostRoute route = ToDeviceRouteFor(facts);
		lastRoute = (int)route;
		switch (route)
		{
		case HostRoute::ToDeviceInPlace:
			ProcessDeviceOrdered(dStage, dOut, n, (long)n, outStride);
			break;
		case HostRoute::ToDeviceCopies:
			CheckHip(hipMemcpyAsync(devStage, hostStage, total * sizeof(float), hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
			ProcessDeviceOrdered(devStage, dOut, n, (long)n, outStride);
			break;
		default:
			throw std::logic_error("neuralaudio_amd: internal: ProcessHostToDevice route");
		}
	}

	// the three events of a slot; true: they were created now (the slot's first use)
	bool GpuBatch::EnsureSlotEvents(PipeSlot& p)
	{
		if (p.uploaded) return false;
		CheckHip(CountedHipEventCreateWithFlags(&p.uploaded, hipEventDisableTiming), "hipEventCreate");
		CheckHip(CountedHipEventCreateWithFlags(&p.computed, hipEventDisableTiming), "hipEventCreate");
		CheckHip(CountedHipEventCreateWithFlags(&p.downloaded, hipEventDisableTiming), "hipEventCreate");
		return true;
	}

	void GpuBatch::EnsurePipeSlot(PipeSlot& p, size_t floats)
	{
		if (EnsureSlotEvents(p))
		{
			// the set-up side of the pipelined interface: the half-batch chains' streams too (creating a HIP stream takes ~13 ms)
			for (int h = 0; h < numChains; h++)
				if (!halfStream[h]) CheckHip(CountedHipStreamCreateWithFlags(&halfStream[h], hipStreamNonBlocking), "hipStreamCreate");
		}
		if (floats <= p.floats) return;
		if (p.hostIn) (void)CountedHipHostFree(p.hostIn);
		if (p.hostOut) (void)CountedHipHostFree(p.hostOut);
		if (p.dev) (void)CountedHipFree(p.dev);
		p.hostIn = p.hostOut = p.dev = nullptr;
		p.floats = 0;
		CheckHip(CountedHipHostMalloc(reinterpret_cast<void**>(&p.hostIn), floats * sizeof(float), hipHostMallocDefault), "hipHostMalloc");
		CheckHip(CountedHipHostMalloc(reinterpret_cast<void**>(&p.hostOut), floats * sizeof(float), hipHostMallocDefault), "hipHostMalloc");
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&p.dev), floats * sizeof(float)), "hipMalloc");
		p.floats = floats;
	}

	// The pool's share of the pipelined interface's set-up side: every stream and event that Submit / Collect, or an ordered call behind
	// them, creates on first use.  Which of them a buffer needs depends on the number of launch units (one: the slots' own streams;
	// several, or a resampling batch: the copy streams), and an activation or a park may change that number on a running batch.
	void GpuBatch::EnsurePoolPipeline()
	{
		for (PipeSlot& p : pipe)
		{
			(void)EnsureSlotEvents(p);
			if (!p.own) CheckHip(CountedHipStreamCreateWithFlags(&p.own, hipStreamNonBlocking), "hipStreamCreate");
			for (int h = 0; h < numChains; h++)
				if (!p.halfDone[h]) CheckHip(CountedHipEventCreateWithFlags(&p.halfDone[h], hipEventDisableTiming), "hipEventCreate");
		}
		for (int h = 0; h < numChains; h++)
			if (!halfStream[h]) CheckHip(CountedHipStreamCreateWithFlags(&halfStream[h], hipStreamNonBlocking), "hipStreamCreate");
		if (!copyIn) CheckHip(CountedHipStreamCreateWithFlags(&copyIn, hipStreamNonBlocking), "hipStreamCreate");
		if (!copyOut) CheckHip(CountedHipStreamCreateWithFlags(&copyOut, hipStreamNonBlocking), "hipStreamCreate");
		inFlight->EnsureMainDone();
	}

	int GpuBatch::Submit(const float* in, size_t n)
	{
		CheckUsable();
		if (n == 0 || streams.empty()) throw std::runtime_error("neuralaudio_amd: Submit on an empty batch / buffer");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		const int ticket = nextSlot;
		PipeSlot& p = pipe[ticket];
		if (p.busy) throw std::runtime_error("neuralaudio_amd: Submit with every pipeline slot in flight (Collect the oldest ticket first)");
		FlushRearms();
		const size_t total = streams.size() * n;
		EnsurePipeSlot(p, total);
		p.n = n;
		p.rows = streams.size(); // Collect sizes its copy by THIS (AddStreams / RemoveStreams may run while the ticket is in flight)
		p.parkedRows.clear(); // (a stream may join or leave while the ticket is in flight: the rows parked NOW are this buffer's silent ones)
		if (numParked > 0)
			for (size_t r = 0; r < streams.size(); r++)
				if (streams[r].parked) p.parkedRows.push_back((int)r);
		if (in) memcpy(p.hostIn, in, total * sizeof(float)); // nullptr: the caller filled NextInput() in place
		SubmitFacts facts = {};
		facts.hostDirect = HostDirect();
		facts.stageEntries = StageHasEntries();
		facts.resamples = Resamples();
		float *dIn = nullptr, *dOut = nullptr;
		if (DirectRows(facts.hostDirect, facts.stageEntries)) // (no read-modify-write over the bus: see ProcessHost)
		{
			dIn = DeviceAlias(p.hostIn);
			dOut = DeviceAlias(p.hostOut);
		}
		facts.pinnedAddressable = dIn && dOut;
		facts.callerPassedIn = in != nullptr;
		for (const PipeSlot& o : pipe) facts.otherTicketInFlight = facts.otherTicketInFlight || (&o != &p && o.busy);
		facts.chainsInUse = inFlight->halfChainsUsed;
		UpdatePlan();
		facts.launchUnits = (int)plan.units.size();
		const HostRoute route = SubmitRouteFor(facts, SubmitTriesHalves(facts) && PrepareHalves(n));
		lastRoute = (int)route;
		switch (route)
		{
		case HostRoute::SubmitHalves:
			// two free-running half-batch chains (see halfStream): each half in submission order on its own stream
			for (int h = 0; h < numChains; h++)
				if (!p.halfDone[h]) CheckHip(CountedHipEventCreateWithFlags(&p.halfDone[h], hipEventDisableTiming), "hipEventCreate");
			LaunchHalves(dIn, dOut, n, (long)n, (long)n, p.halfDone, true);
			inFlight->halfChainsUsed = true;
			inFlight->NoteNoLastKernel(); // (ProcessDevice after this drains the half streams itself)
			p.wait = SlotWait::ChainEvents;
			break;
		case HostRoute::SubmitInPlace:
			JoinHalves(); // back on the batch stream: the half chains first
			// (the buffer before this one ran on its slot's own stream while the output stage had entries: this buffer's kernel, and any
			// index list it uploads again, come behind that one's)
			inFlight->OrderBehindLastKernel(stream);
			ProcessDeviceOn(stream, dIn, dOut, n, (long)n, (long)n);
			inFlight->lastSubmitOnBatchStream = true;
			CheckHip(hipEventRecord(p.downloaded, stream), "hipEventRecord");
			p.wait = SlotWait::DownloadedEvent;
			break;
		case HostRoute::SubmitOwnStream:
		{
			// One launch per buffer (the usual case): the whole buffer -- upload, kernel, download -- rides on the slot's OWN stream, in order,
			// with no event between them; the only cross-stream edge is the stream state: this buffer's kernel waits for the previous
			// buffer's.  The upload of buffer k + 1 (its stream's first operation) overlaps the kernel of buffer k, the download of buffer k
			// (behind its kernel) overlaps the kernel of buffer k + 1.  Per buffer: 2 copies, 1 launch, 1 event wait, 1 event record --
			// the round-2 path cost 2 more waits and 2 more records on the compute stream, 15 us per buffer (tools/microbench/host_pipe_probe.cpp).
			JoinHalves(); // (device-pointer steps may have run as half-batch chains: this buffer's kernel comes after both)
			if (!p.own) CheckHip(CountedHipStreamCreateWithFlags(&p.own, hipStreamNonBlocking), "hipStreamCreate");
			bool listsChanged = false, dirty = false;
			for (auto& g : groups) dirty = dirty || (g->NumActive() > 0 && g->ListsDirty());
			if (dirty)
			{
				// the index lists are re-uploaded on the batch stream: not before the kernels still reading the old ones are done
				inFlight->OrderBehindLastKernel(stream);
				for (auto& g : groups)
					if (g->NumActive() > 0) listsChanged = g->SyncActiveLists() || listsChanged;
			}
			if (listsChanged || inFlight->submitTopology != topologyVersion || !inFlight->pipelineUsed || inFlight->lastSubmitOnBatchStream)
			{
				// everything the batch stream still has in flight for this batch (state resets of new streams, index lists, the buffer
				// before this one where it ran there: the output stage's first entry moves the buffers of a direct batch over here) comes first
				CheckHip(hipStreamWaitEvent(p.own, inFlight->RecordMainDone(stream), 0), "hipStreamWaitEvent");
				inFlight->submitTopology = topologyVersion;
				inFlight->lastSubmitOnBatchStream = false;
			}
			inFlight->pipelineUsed = true;
			CheckHip(hipMemcpyAsync(p.dev, p.hostIn, total * sizeof(float), hipMemcpyHostToDevice, p.own), "hipMemcpyAsync H2D");
			inFlight->OrderBehindLastKernel(p.own);
			ProcessDeviceOn(p.own, p.dev, p.dev, n, (long)n, (long)n);
			CheckHip(hipEventRecord(p.computed, p.own), "hipEventRecord");
			inFlight->NoteLastKernel(p.computed, p.own);
			CheckHip(hipMemcpyAsync(p.hostOut, p.dev, total * sizeof(float), hipMemcpyDeviceToHost, p.own), "hipMemcpyAsync D2H");
			p.wait = SlotWait::OwnStream;
			break;
		}
		case HostRoute::SubmitCopyStreams:
			// several launch units per buffer (a captured hipGraph on the batch stream): copies on the copy streams, events in between
			if (!copyIn)
			{
				CheckHip(CountedHipStreamCreateWithFlags(&copyIn, hipStreamNonBlocking), "hipStreamCreate");
				CheckHip(CountedHipStreamCreateWithFlags(&copyOut, hipStreamNonBlocking), "hipStreamCreate");
			}
			CheckHip(hipMemcpyAsync(p.dev, p.hostIn, total * sizeof(float), hipMemcpyHostToDevice, copyIn), "hipMemcpyAsync H2D");
			CheckHip(hipEventRecord(p.uploaded, copyIn), "hipEventRecord");
			CheckHip(hipStreamWaitEvent(stream, p.uploaded, 0), "hipStreamWaitEvent");
			ProcessDeviceOrdered(p.dev, p.dev, n, (long)n, (long)n);
			CheckHip(hipEventRecord(p.computed, stream), "hipEventRecord");
			CheckHip(hipStreamWaitEvent(copyOut, p.computed, 0), "hipStreamWaitEvent");
			CheckHip(hipMemcpyAsync(p.hostOut, p.dev, total * sizeof(float), hipMemcpyDeviceToHost, copyOut), "hipMemcpyAsync D2H");
			CheckHip(hipEventRecord(p.downloaded, copyOut), "hipEventRecord");
			p.wait = SlotWait::DownloadedEvent;
			break;
		default:
			throw std::logic_error("neuralaudio_amd: internal: Submit route");
		}
		p.busy = true;
		nextSlot = (nextSlot + 1) % kPipelineSlots;
		return ticket;
	}

	void GpuBatch::Collect(int ticket, float* out)
	{
		CheckUsable();
		if (ticket < 0 || ticket >= kPipelineSlots || !pipe[ticket].busy) throw std::runtime_error("neuralaudio_amd: Collect with an invalid ticket");
		PipeSlot& p = pipe[ticket];
		switch (p.wait)
		{
		case SlotWait::ChainEvents:
			for (int h = 0; h < numChains; h++) WaitEventBounded(p.halfDone[h], "hipEventSynchronize");
			break;
		case SlotWait::OwnStream:
			WaitStreamBounded(p.own, "hipStreamSynchronize"); // the download is the stream's last operation
			break;
		case SlotWait::DownloadedEvent:
			WaitEventBounded(p.downloaded, "hipEventSynchronize");
			break;
		}
		// the slot holds the rows the batch had at Submit: ids retired since then are zeroed only inside that block
		for (int id : retired)
			if ((size_t)id < p.rows) memset(p.hostOut + (size_t)id * p.n, 0, p.n * sizeof(float));
		for (int r : p.parkedRows) memset(p.hostOut + (size_t)r * p.n, 0, p.n * sizeof(float));
		if (out) memcpy(out, p.hostOut, p.rows * p.n * sizeof(float)); // nullptr: the caller reads OutputView() in place
		p.busy = false;
	}

	float* GpuBatch::NextInput(size_t n)
	{
		CheckUsable();
		if (n == 0 || streams.empty()) throw std::runtime_error("neuralaudio_amd: NextInput on an empty batch / buffer");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		PipeSlot& p = pipe[nextSlot];
		if (p.busy) throw std::runtime_error("neuralaudio_amd: NextInput with every pipeline slot in flight (Collect the oldest ticket first)");
		EnsurePipeSlot(p, streams.size() * n);
		return p.hostIn;
	}

	const float* GpuBatch::OutputView(int ticket) const
	{
		if (ticket < 0 || ticket >= kPipelineSlots) throw std::runtime_error("neuralaudio_amd: OutputView with an invalid ticket");
		return pipe[ticket].hostOut;
	}

}
