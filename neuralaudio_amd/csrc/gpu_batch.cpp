// gpu_batch.cpp -- see gpu_batch.h.  Host side only: device memory, tables, launches.
#include "gpu_batch.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <mutex>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include <hip/hip_runtime.h>

#include "gpu_batch_internal.h"

namespace na
{
	void CheckHip(hipError_t e, const char* what)
	{
		if (e != hipSuccess) throw HipError(e, what);
	}

	static std::atomic<long long> gDeviceResourceCalls{ 0 };
	void CountDeviceResourceCall() { gDeviceResourceCalls.fetch_add(1, std::memory_order_relaxed); }
	long long DeviceResourceCalls() { return gDeviceResourceCalls.load(std::memory_order_relaxed); }

	int VisibleDeviceCount()
	{
		int count = 0;
		const hipError_t e = hipGetDeviceCount(&count);
		if (e != hipSuccess)
		{
			(void)hipGetLastError();
			return 0;
		}
		return count;
	}

}

namespace na
{
	// Host side only (no device): which kernel family a batch would pick for `streams` streams of this submodel -- what its WaveNetGroup
	// would ask (wavenet_choice.h WaveNetKernelFor) -- and the facts of the range proof behind the choice.
	ModelKernelInfo PredictModelKernel(const LoadedModel& model, float quality, int streams)
	{
		ModelKernelInfo info;
		if (model.subModels.empty()) return info;
		const int idx = model.isComposite ? model.ModelIndexFromQuality(quality) : 0;
		const ModelDesc& d = *model.subModels[(size_t)idx].desc;
		if (d.kind != MODEL_WAVENET)
		{
			info.kernel = "recurrent";
			return info;
		}
		const int packHint = (!model.isComposite && model.subModels.size() == 1) ? streams : 0;
		const WaveNetGroupChoice c = WaveNetKernelFor(d.wavenet, packHint, WaveNetKnobs::FromTuning());
		info.kernel = c.FamilyName();
		info.pack = c.pack;
		info.inputLimit = c.inputLimit;
		info.rangeProven = c.rangeProven;
		info.weightsOk = c.weightsOk;
		return info;
	}

	// Cost of one stream for the multi-GPU sharder: time = per-launch skeleton + bytes (WaveNet) / multiply-accumulates (recurrent),
	// two-point fits per kernel family to the round-3 measurements (us per 1024 streams x 128 frames): specialised / split chains
	// 22.3 + 0.0143 B (Standard 41.6, Lite 33.7), f32 frame kernel 31.6 + 0.0164 B (A2-Lite 46.6, A2-Full 71.4), LDS-free recurrent
	// kernel 8.4 + 0.0107 MAC (LSTM 1x16 20.2, 2x16 42.1), runtime-shaped kernels by their measured per-block times.
	double EstimateStreamCost(const LoadedModel& model, float quality)
	{
		if (model.subModels.empty()) return 1.0;
		const int idx = model.isComposite ? model.ModelIndexFromQuality(quality) : 0;
		const ModelDesc& d = *model.subModels[(size_t)idx].desc;
		if (d.kind == MODEL_WAVENET)
		{
			const WaveNetPlan plan = BuildWaveNetPlan(d.wavenet, true);
			const double B = plan.AlgorithmicBytesPerSample(WN_MAX_FRAMES);
			if (plan.genericOnly) return 1000.0 * plan.maxChannels / 32.0; // 1.0 ms per block at 32 channels (<= 256 streams)
			const bool composite = model.isComposite;
			// (deliberately the fit's own predicate, not the dispatch's -- wavenet_choice.h WaveNetKernelFor: the fit was made against it)
			const bool split = plan.splitFastT == 2 || (!composite && (WaveNetPackFactor(d.wavenet) > 1 || WaveNetWantsPadding(d.wavenet)));
			return split ? 22.3 + 0.0143 * B : 31.6 + 0.0164 * B;
		}
		const LSTMDesc& l = d.lstm;
		const double gates = (l.cell == CELL_GRU) ? 3.0 : 4.0;
		double macs = 0.0;
		for (int k = 0; k < l.numLayers; k++) macs += gates * l.hiddenSize * ((k == 0 ? 1 : l.hiddenSize) + l.hiddenSize);
		macs += l.hiddenSize;
		const bool dpp = l.tail.empty() && l.numLayers <= 2 && (l.hiddenSize <= 16 || (l.numLayers == 1 && l.hiddenSize <= 32));
		return dpp ? 8.4 + 0.0107 * macs : 60.0 + 0.06 * macs;
	}

	// ------------------------------------------------------------------------------------------ GpuBatch

	GpuBatch::GpuBatch(int dev, hipStream_t borrowedStream) : device(dev), inFlight(new InFlight())
	{
		const int count = VisibleDeviceCount();
		if (count <= 0) throw std::runtime_error("neuralaudio_amd: no HIP device is visible; this library has no CPU fallback");
		if (dev < 0 || dev >= count) throw std::runtime_error("neuralaudio_amd: invalid HIP device index");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (borrowedStream)
		{
			stream = borrowedStream;
			ownsStream = false;
			streamObserved = true; // the caller orders its own work on it
		}
		else
		{
			CheckHip(CountedHipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
		}
		numChains = std::min(std::max(Tuning::Get().hostChains, 2), kMaxChains);
	}

	GpuBatch::~GpuBatch()
	{
		(void)hipSetDevice(device);
		// everything this batch has in flight, under the wait limit (gpu_batch.h "bounded waits").  A device that does not come back keeps
		// the allocations: a kernel that is still running may write them, and hipFree would wait for it without a limit.
		bool idle = true;
		try
		{
			if (broken)
			{
				// (the resident launch of a broken batch: asked to leave, not waited for command by command)
				if (residentState && residentState->ctrl) __atomic_store_n(&residentState->ctrl->exitAfter, 0ull, __ATOMIC_RELEASE);
			}
			else DrainResident();
			for (PipeSlot& p : pipe)
				if (p.own) WaitStreamBounded(p.own, "closing the batch");
			for (hipStream_t hs : halfStream)
				if (hs) WaitStreamBounded(hs, "closing the batch");
			if (stream) WaitStreamBounded(stream, "closing the batch");
		}
		catch (...)
		{
			idle = false;
		}
		if (!idle)
		{
			for (auto& g : groups) (void)g.release();
			(void)residentState.release();
			(void)resample.release();
			for (auto& stage : stages) (void)stage.release();
			for (WnLaunchTable& t : wnTable) t.entries.clear();
			return;
		}
		residentState.reset();
		groups.clear();
		if (hostStage) (void)CountedHipHostFree(hostStage);
		if (devStage) (void)CountedHipFree(devStage);
		if (snapHost) (void)CountedHipHostFree(snapHost);
		if (snapDev) (void)CountedHipFree(snapDev);
		for (PipeSlot& p : pipe)
		{
			if (p.hostIn) (void)CountedHipHostFree(p.hostIn);
			if (p.hostOut) (void)CountedHipHostFree(p.hostOut);
			if (p.dev) (void)CountedHipFree(p.dev);
			if (p.uploaded) (void)hipEventDestroy(p.uploaded);
			if (p.computed) (void)hipEventDestroy(p.computed);
			if (p.downloaded) (void)hipEventDestroy(p.downloaded);
			for (hipEvent_t e : p.halfDone)
				if (e) (void)hipEventDestroy(e);
			if (p.own) (void)hipStreamDestroy(p.own);
		}
		if (inFlight->mainDone) (void)hipEventDestroy(inFlight->mainDone);
		for (hipStream_t hs : halfStream)
			if (hs) (void)hipStreamDestroy(hs);
		for (auto& m : marks)
			for (hipEvent_t e : m)
				if (e) (void)hipEventDestroy(e);

		if (copyIn) (void)hipStreamDestroy(copyIn);
		if (copyOut) (void)hipStreamDestroy(copyOut);
		for (auto& e : graphCache) (void)hipGraphExecDestroy(e.exec);
		if (forkEvent) (void)hipEventDestroy(forkEvent);
		if (stream && ownsStream) (void)hipStreamDestroy(stream);
	}

	ModelGroup* GpuBatch::GroupFor(const std::shared_ptr<const ModelDesc>& desc, int packHint)
	{
		for (auto& g : groups)
			if (g->desc.get() == desc.get()) return g.get();
		CheckHip(hipSetDevice(device), "hipSetDevice");
		std::unique_ptr<ModelGroup> g;
		if (desc->kind == MODEL_WAVENET) g.reset(new WaveNetGroup(desc, stream, packHint, peerWeights));
		else if (desc->kind == MODEL_LSTM) g.reset(new LstmGroup(desc, stream, peerWeights));
		else throw std::runtime_error("neuralaudio_amd: unsupported model kind");
		if (peerWeights) awaitingWeights.push_back(g.get());
		groups.push_back(std::move(g));
		return groups.back().get();
	}

	int GpuBatch::AddStream(const std::shared_ptr<const LoadedModel>& model, float quality, bool prewarm, bool onDemand)
	{
		return AddStreams(model, quality, 1, prewarm, onDemand);
	}

	// ids for `count` new streams: retired ones first (the lowest for a single stream, a run of consecutive ones for several), else new rows
	int GpuBatch::AllocateIds(int count)
	{
		for (size_t i = 0; i + (size_t)count <= retired.size(); i++)
		{
			if (retired[i + (size_t)count - 1] == retired[i] + count - 1)
			{
				const int first = retired[i];
				retired.erase(retired.begin() + (long)i, retired.begin() + (long)i + count);
				return first;
			}
		}
		const int first = (int)streams.size();
		streams.resize(streams.size() + (size_t)count);
		for (int i = 0; i < count; i++) streams[(size_t)(first + i)].live = false;
		return first;
	}

	int GpuBatch::AddStreams(const std::shared_ptr<const LoadedModel>& model, float quality, int count, bool prewarm, bool onDemand)
	{
		return CreateStreams(model, quality, count, prewarm, onDemand, false);
	}

	// `pool`: the streams are created PARKED and armed (ReserveStreams) -- no member active, every submodel prewarmed or none
	int GpuBatch::CreateStreams(const std::shared_ptr<const LoadedModel>& model, float quality, int count, bool prewarm, bool onDemand, bool pool)
	{
		CheckUsable();
		if (!model || model->subModels.empty()) throw std::runtime_error("neuralaudio_amd: AddStream with an empty model");
		if (count < 1) throw std::runtime_error("neuralaudio_amd: AddStreams with count < 1");
		if (resample) CheckResampleModelRate(model->ProcessRate(), resample->plan.modelRate);
		if (pool && (peerWeights || AwaitsWeights())) throw std::runtime_error("neuralaudio_amd: ReserveStreams: the batch takes its weights from a peer device (pools are not part of the multi-GPU host)");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		DrainPipeline(); // (state arrays may be re-allocated below)
		topologyVersion++;
		const int active = model->isComposite ? model->ModelIndexFromQuality(quality) : 0;
		const size_t numSub = model->subModels.size();
		std::vector<ModelGroup*> subGroups(numSub);
		std::vector<std::vector<int>> newMembers(numSub);
		for (size_t k = 0; k < numSub; k++) subGroups[k] = GroupFor(model->subModels[k].desc, (!model->isComposite && numSub == 1) ? count : 0);
		const int first = AllocateIds(count);
		// Everything below may throw (hipMalloc inside AddMember / Reset / Prewarm).  A failed call must leave the batch as it was: the
		// members it created are removed again, the ids go back to `retired` (rows appended by AllocateIds leave the arrays).
		int built = 0; // rows [first, first + built) are complete StreamRefs
		std::vector<std::pair<ModelGroup*, int>> partial; // members of the row under construction
		const size_t pendingBefore = pendingPrewarm.size(); // (deferred prewarms this call files: dropped again if it fails)
		try
		{
			for (int i = 0; i < count; i++)
			{
				StreamRef ref;
				ref.model = model;
				ref.quality = quality;
				ref.active = active;
				ref.onDemand = onDemand;
				ref.live = true;
				ref.prewarmed.assign(numSub, 0);
				const int row = first + i;
				partial.clear();
				for (size_t k = 0; k < numSub; k++)
				{
					const int member = subGroups[k]->AddMember();
					partial.push_back({ subGroups[k], member });
					newMembers[k].push_back(member);
				}
				ref.members = partial;
				partial.clear();
				ref.pooled = ref.parked = pool;
				ref.poolPrewarm = pool && prewarm;
				if (!pool) ref.members[(size_t)active].first->SetActive(ref.members[(size_t)active].second, row);
				streams[(size_t)row] = ref;
				built = i + 1;
			}
			// fresh state for every new member, then prewarm: every submodel (LoadAll, CompositeModel.h:111-118) or only the active one
			// (OnDemand, :104-109 -- the others are prewarmed when a quality change first selects them, :52-60)
			for (size_t k = 0; k < numSub; k++)
			{
				std::sort(newMembers[k].begin(), newMembers[k].end());
				if (pool)
				{
					subGroups[k]->ArmReserved(newMembers[k], prewarm);
					for (int i = 0; i < count; i++) streams[(size_t)(first + i)].prewarmed[k] = prewarm ? 1 : 0;
					continue;
				}
				subGroups[k]->Reset(newMembers[k]);
				const bool now = prewarm && (!onDemand || (int)k == active);
				const bool waits = now && std::find(awaitingWeights.begin(), awaitingWeights.end(), subGroups[k]) != awaitingWeights.end();
				if (waits) pendingPrewarm.push_back({ subGroups[k], newMembers[k] }); // (its weights are not on the device yet: WeightsArrived)
				else if (now) subGroups[k]->Prewarm(newMembers[k]);
				for (int i = 0; i < count; i++) streams[(size_t)(first + i)].prewarmed[k] = now ? 1 : 0;
			}
			if (Resamples())
			{
				// history slots for every row, on this, the set-up side; a new or recycled stream starts from zero histories
				EnsureResampleRows((int)streams.size());
				ZeroResampleHistories(first, count);
			}
		}
		catch (...)
		{
			pendingPrewarm.resize(pendingBefore); // (WeightsArrived must not prewarm member slots that are gone or recycled)
			for (auto& gm : partial) gm.first->RemoveMember(gm.second);
			for (int i = 0; i < count; i++)
			{
				StreamRef& ref = streams[(size_t)(first + i)];
				if (i < built)
					for (auto& gm : ref.members) gm.first->RemoveMember(gm.second);
				ref = StreamRef();
				ref.live = false;
				retired.insert(std::lower_bound(retired.begin(), retired.end(), first + i), first + i);
			}
			DropTrailingRetiredRows();
			throw;
		}
		// the half-batch chains' streams on this, the set-up side (creating a HIP stream takes ~13 ms: not inside the first buffer)
		if (ownsStream && !streamObserved && streams.size() >= 512)
			for (int h = 0; h < numChains; h++)
				if (!halfStream[h]) CheckHip(CountedHipStreamCreateWithFlags(&halfStream[h], hipStreamNonBlocking), "hipStreamCreate");
		if (pool)
		{
			numParked += count;
			// what a later activation or park may be the first to need: the side streams and events of a batch of several launch units,
			// and the pipelined interface's streams and events for either number of units (an activation may add a unit, a park take one away)
			if (groups.size() > 1)
			{
				for (auto& g : groups)
				{
					(void)g->SideStream();
					(void)g->DoneEvent();
				}
				if (!forkEvent) CheckHip(CountedHipEventCreateWithFlags(&forkEvent, hipEventDisableTiming), "hipEventCreate");
			}
			EnsurePoolPipeline();
			pendingHistoryZero.reserve(streams.size());
		}
		for (auto& stage : stages)
			if (stage) stage->EnsureRows(*this, (int)streams.size());
		return first;
	}

	int GpuBatch::ReserveStreams(const std::shared_ptr<const LoadedModel>& model, int count, bool prewarm)
	{
		return CreateStreams(model, 1.0f, count, prewarm, false, true);
	}

	int GpuBatch::FindParked(const LoadedModel* model) const
	{
		for (size_t s = 0; s < streams.size(); s++)
			if (streams[s].parked && streams[s].model.get() == model) return (int)s;
		return -1;
	}

	// Real-time safe: host bookkeeping only.  The device work -- list upload, re-arm, zero histories -- is enqueued by the next processing
	// call (FlushRearms, SyncActiveLists).
	void GpuBatch::ActivateStream(int s, float quality)
	{
		CheckUsable();
		if (!IsParked(s)) throw std::runtime_error("neuralaudio_amd: ActivateStream: stream " + std::to_string(s) + " is not a parked stream of the batch");
		StreamRef& ref = streams[(size_t)s];
		ref.quality = quality;
		ref.active = ref.model->isComposite ? ref.model->ModelIndexFromQuality(quality) : 0;
		// It must start armed.  A stream that ran since it was armed is armed again, every submodel (a quality switch may have run any of
		// them); so is every member of a packed group: its virtual stream may have been running for its neighbours, with this
		// position's channel groups taking zero input along
		for (auto& gm : ref.members)
			if (ref.used || gm.first->PackFactor() > 1)
			{
				gm.first->QueueRearm(gm.second, ref.poolPrewarm);
				rearmPending = true;
			}
		for (size_t k = 0; k < ref.prewarmed.size(); k++) ref.prewarmed[k] = ref.poolPrewarm ? 1 : 0;
		ref.members[(size_t)ref.active].first->SetActive(ref.members[(size_t)ref.active].second, s);
		if (Resamples())
		{
			pendingHistoryZero.push_back(s); // (a joining stream starts from zero filter histories at the batch's current phase)
			rearmPending = true;
		}
		ref.parked = false;
		ref.used = true;
		numParked--;
		topologyVersion++;
	}

	void GpuBatch::ParkStream(int s)
	{
		CheckUsable();
		if (IsParked(s)) throw std::runtime_error("neuralaudio_amd: ParkStream: stream " + std::to_string(s) + " is parked already");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: ParkStream: stream " + std::to_string(s) + " is not a live stream of the batch");
		StreamRef& ref = streams[(size_t)s];
		if (!ref.pooled) throw std::runtime_error("neuralaudio_amd: ParkStream: stream " + std::to_string(s) + " did not come from ReserveStreams (it leaves through RemoveStreams)");
		ref.members[(size_t)ref.active].first->SetActive(ref.members[(size_t)ref.active].second, -1);
		pendingHistoryZero.erase(std::remove(pendingHistoryZero.begin(), pendingHistoryZero.end(), s), pendingHistoryZero.end());
		StageLeave(s);
		ref.parked = true;
		numParked++;
		topologyVersion++;
	}

	// The device side of ActivateStream, on the batch stream in front of the model launches (and of the list uploads): one re-arm launch
	// per model group with members waiting, the asynchronous zeroing of the activated rows' filter histories.  Behind whatever of the
	// batch may still touch those slots: the pipelined slots' kernels by an event; half-batch chains and the resident launch are drained
	// (the one host-side wait, shared with a quality switch on such a batch -- bounded by the wait limit).
	void GpuBatch::FlushRearms()
	{
		if (stages[kOutputStage]) StageParkFinished();
		if (!rearmPending) return;
		JoinHalves();
		inFlight->OrderBehindLastKernel(stream);
		for (auto& g : groups) g->FlushRearm();
		for (int s : pendingHistoryZero) ZeroResampleHistories(s, 1);
		pendingHistoryZero.clear();
		rearmPending = false;
	}

	// trailing retired rows leave the [streams][n] arrays altogether (their ids are the largest entries of the sorted `retired` list)
	void GpuBatch::DropTrailingRetiredRows()
	{
		while (!streams.empty() && !streams.back().live)
		{
			if (!retired.empty() && retired.back() == (int)streams.size() - 1) retired.pop_back();
			streams.pop_back();
		}
	}

	hipStream_t GpuBatch::GetStream()
	{
		if (!streamObserved)
		{
			(void)hipSetDevice(device);
			JoinHalves();
			streamObserved = true;
		}
		return stream;
	}

	void GpuBatch::RemoveStreams(int first, int count)
	{
		CheckUsable();
		if (count < 1 || first < 0 || (size_t)first + (size_t)count > streams.size()) throw std::runtime_error("neuralaudio_amd: RemoveStreams: id range outside the batch");
		for (int i = 0; i < count; i++)
			if (!streams[(size_t)(first + i)].live) throw std::runtime_error("neuralaudio_amd: RemoveStreams: stream was already removed");
		// (a parked stream is freed like any other: its slots, its pending re-arm, its place in the pool)
		CheckHip(hipSetDevice(device), "hipSetDevice");
		// the slots may be handed out again right away: nothing of theirs may still be in flight
		Quiesce();
		topologyVersion++;
		for (int i = 0; i < count; i++)
		{
			StreamRef& ref = streams[(size_t)(first + i)];
			for (auto& gm : ref.members) gm.first->RemoveMember(gm.second);
			if (ref.parked) numParked--;
			pendingHistoryZero.erase(std::remove(pendingHistoryZero.begin(), pendingHistoryZero.end(), first + i), pendingHistoryZero.end());
			StageLeave(first + i);
			ref = StreamRef();
			ref.live = false;
			retired.insert(std::lower_bound(retired.begin(), retired.end(), first + i), first + i);
		}
		DropTrailingRetiredRows();
	}

	unsigned GpuBatch::StreamPrewarmedMask(int s) const
	{
		const StreamRef& ref = streams.at((size_t)s);
		unsigned mask = 0;
		for (size_t k = 0; k < ref.prewarmed.size() && k < 32; k++) mask |= ref.prewarmed[k] ? (1u << k) : 0u;
		return mask;
	}

	void GpuBatch::ZeroRetiredRows(float* hostRows, size_t n, size_t rows) const
	{
		for (int id : retired)
			if ((size_t)id < rows) memset(hostRows + (size_t)id * n, 0, n * sizeof(float));
		if (numParked > 0)
			for (size_t id = 0; id < rows && id < streams.size(); id++)
				if (streams[id].parked) memset(hostRows + id * n, 0, n * sizeof(float));
	}

	void GpuBatch::SetQuality(int s, float quality)
	{
		CheckUsable();
		StreamRef& ref = streams.at((size_t)s);
		if (!ref.live) throw std::runtime_error("neuralaudio_amd: stream was removed");
		if (ref.parked) throw std::runtime_error("neuralaudio_amd: SetQuality: stream " + std::to_string(s) + " is parked (ActivateStream takes the quality)");
		ref.quality = quality;
		if (!ref.model->isComposite) return;
		const int idx = ref.model->ModelIndexFromQuality(quality);
		if (idx == ref.active) return;
		ref.members[(size_t)ref.active].first->SetActive(ref.members[(size_t)ref.active].second, -1);
		ref.active = idx;
		ref.members[(size_t)idx].first->SetActive(ref.members[(size_t)idx].second, s);
		topologyVersion++;
		if (ref.onDemand && !ref.prewarmed[(size_t)idx])
		{
			// CompositeModel::SetCurrentModelIndex (CompositeModel.h:52-60): first use of this submodel -- NOT real-time safe, which
			// IsQualityChangeRealtimeSafe() reports beforehand
			Quiesce(); // (the prewarm runs on the batch stream: behind a resident launch it would wait for that to idle out)
			ref.members[(size_t)idx].first->Prewarm({ ref.members[(size_t)idx].second });
			ref.prewarmed[(size_t)idx] = 1;
		}
	}

	std::vector<LaunchKind> GpuBatch::ActiveKinds(const ModelGroup* leaving, const ModelGroup* entering, std::vector<ModelGroup*>* active) const
	{
		std::vector<LaunchKind> kinds;
		for (const auto& g : groups)
		{
			if (g->NumActive() - (g.get() == leaving) + (g.get() == entering) <= 0) continue;
			kinds.push_back(g->Kind());
			if (active) active->push_back(g.get());
		}
		return kinds;
	}

	// (every change of which groups have active streams -- AddStreams, RemoveStreams, SetQuality -- is a new topology version)
	void GpuBatch::UpdatePlan()
	{
		if (plan.version == topologyVersion) return;
		plan.groups.clear();
		plan.units = PlanLaunches(ActiveKinds(nullptr, nullptr, &plan.groups));
		plan.version = topologyVersion;
	}

	// The groups of a frame / split / packed unit as its launch takes them -- a plain group in the packed launch passes its index lists
	// (launch_plan.h) -- in the unit's order, or in group order (the lists of the half-batch chains and of the resident launch keep the
	// joiners where they stand).  The unit's kind makes every one of them a WaveNetGroup.
	std::vector<WnFrameGroup> GpuBatch::WaveNetArgs(const LaunchUnit& unit, bool groupOrder)
	{
		std::vector<int> sorted;
		if (groupOrder)
		{
			sorted = unit.groups;
			std::sort(sorted.begin(), sorted.end());
		}
		std::vector<WnFrameGroup> args;
		args.reserve(unit.groups.size());
		for (int i : groupOrder ? sorted : unit.groups)
			args.push_back(static_cast<WaveNetGroup*>(plan.groups[(size_t)i])->LaunchArgs(unit.kind == LaunchKind::SplitPacked));
		return args;
	}

	// CompositeModel::IsModelChangeRealtimeSafe (CompositeModel.h:44-50, HadInitialPrewarm): false when the target submodel never had its
	// prewarm -- the switch would prewarm it (OnDemand) or run it cold (a stream added without prewarm) -- and false when the batch
	// would take several launches per buffer afterwards: those run as a captured hipGraph, which a switch re-captures.  Otherwise a
	// switch only re-uploads two pinned index lists asynchronously.
	bool GpuBatch::IsQualityChangeRealtimeSafe(int s, float quality) const
	{
		const StreamRef& ref = streams.at((size_t)s);
		if (!ref.live || ref.parked) return false;
		if (!ref.model->isComposite) return true;
		const int idx = ref.model->ModelIndexFromQuality(quality);
		if (idx == ref.active) return true;
		if (!ref.prewarmed[(size_t)idx]) return false;
		return PlanLaunches(ActiveKinds(ref.members[(size_t)ref.active].first, ref.members[(size_t)idx].first)).size() <= 1;
	}

	float GpuBatch::GetQuality(int s) const { return streams.at((size_t)s).quality; }
	int GpuBatch::GetActiveSubModel(int s) const { return streams.at((size_t)s).active; }

	void GpuBatch::Prewarm(int s)
	{
		CheckUsable();
		if (IsParked(s)) throw std::runtime_error("neuralaudio_amd: Prewarm: stream " + std::to_string(s) + " is parked (a parked stream is armed already)");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		DrainPipeline();
		StreamRef& ref = streams.at((size_t)s);
		if (!ref.live) return;
		// LoadAll: every submodel is prewarmed (CompositeModel.h:111-118); OnDemand: the current one (:104-109)
		for (size_t k = 0; k < ref.members.size(); k++)
		{
			if (ref.onDemand && (int)k != ref.active) continue;
			ref.members[k].first->Prewarm({ ref.members[k].second });
			ref.prewarmed[k] = 1;
		}
		if (Resamples()) ZeroResampleHistories(s, 1);
	}

	void GpuBatch::ProcessDevice(const float* dIn, float* dOut, size_t n, long inStride, long outStride)
	{
		CheckUsable();
		if (n == 0 || streams.empty()) return;
		CheckHip(hipSetDevice(device), "hipSetDevice");
		FlushRearms();
		// A batch on its own stream that nobody has seen: a buffer of one contiguous WaveNet group runs as two free-running half-batch
		// launches (the order of work on the internal streams is not observable from outside; Synchronize() and the host-buffer entry
		// points wait for all of them).  1024 x A1 Standard x 128 frames: 40.1 -> 37.4 us per step.
		DeviceFacts facts = {};
		facts.ownsStream = ownsStream;
		facts.streamObserved = streamObserved;
		facts.resamples = Resamples();
		facts.stageEntries = StageHasEntries();
		const bool tries = DeviceTriesFreeRunning(facts);
		const bool residentTook = tries && TryResident(dIn, dOut, n, inStride, outStride);
		const HostRoute route = DeviceRouteFor(facts, residentTook, tries && !residentTook && PrepareHalves(n));
		lastRoute = (int)route;
		switch (route)
		{
		case HostRoute::DeviceResident: // (TryResident has posted the command)
			break;
		case HostRoute::DeviceHalves:
			LaunchHalves(dIn, dOut, n, inStride, outStride, nullptr, false);
			break;
		case HostRoute::DeviceOrdered:
			ProcessDeviceOrdered(dIn, dOut, n, inStride, outStride);
			break;
		default:
			throw std::logic_error("neuralaudio_amd: internal: ProcessDevice route");
		}
	}

	// on the batch stream, behind everything launched so far (the host-buffer entry points: their copies are on that stream; a lone
	// blocking buffer gains nothing from two half launches -- 57 vs 60 us)
	void GpuBatch::ProcessDeviceOrdered(const float* dIn, float* dOut, size_t n, long inStride, long outStride)
	{
		lastStepHalves = false;
		lastStepResident = false;
		JoinHalves(); // earlier buffers ran on the resident launch / as two half-batch chains: this call's kernels come after them
		// buffers submitted through the pipelined interface run on per-slot streams: this call's kernels come after theirs ...
		inFlight->OrderBehindLastKernel(stream);
		ProcessDeviceOn(stream, dIn, dOut, n, inStride, outStride);
		// ... and the next submitted buffer after this call's
		if (inFlight->pipelineUsed) inFlight->NoteLastKernel(inFlight->RecordMainDone(stream), stream);
	}

	// One processing call on `launch`, and the one place that states its order: what a stage runs in front of the models, in StageId
	// order -- the gate detector, then the mix stage's stash of the input rows its DRY members name (2.16), then the meter's IN tap (2.14), then the tuner's append and evaluate launches (2.15):
	// they read the input rows as the caller passed them, which may be the output rows, so before any model writes --, the up kernel, the model launches and the down kernel of a
	// resampling batch (ProcessResampledOn) or the model launches alone, then the per-stream stages once per
	// call: behind everything the call has launched -- the join of the units, the graph replay, the down kernel -- on the same stream,
	// outside any capture.  The stages' order is the order of StageId (gpu_batch.h), written there and nowhere else: every row is
	// gated first, then runs through its own EQ cascade (the tone stack sits between amp and cabinet), then is convolved with its own
	// IR (the cabinet's tail rings out through a closing gate), then is compressed by its own level follower and gain curve (dynamics in front of the time-based effects: the compressor stage, 2.19), then is modulated -- chorus, flanger, vibrato, tremolo -- by its own swept line (modulation between dynamics and echo: the modulation stage, 2.20), then runs through its delay line (the echo sits between cabinet and room: the delay stage, 2.18), then runs through its reverb (the room comes behind the cabinet: the reverb stage, 2.17), then is scaled and cross-faded, then the rows of a mix group meet in its
	// output rows (the one stage in which rows meet: behind everything a row goes through on its own); last the meter's OUT and GATE taps read
	// the row the caller receives and the gains the gate applied to it -- they write no audio; the tuner, last in StageId, has nothing
	// left to run there.
	// `launch` != the batch stream is only used for a batch that runs as ONE launch per buffer (Submit checks)
	void GpuBatch::ProcessDeviceOn(hipStream_t launch, const float* dIn, float* dOut, size_t n, long inStride, long outStride)
	{
		for (auto& stage : stages)
			if (stage && stage->HasEntries()) stage->BeforeModels(*this, launch, dIn, n, inStride);
		if (Resamples()) ProcessResampledOn(launch, dIn, dOut, n, inStride, outStride);
		else LaunchModelsOn(launch, dIn, dOut, n, inStride, outStride);
		RunStages(launch, dOut, n, outStride);
	}

	void GpuBatch::RunStages(hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		for (auto& stage : stages)
			if (stage && stage->HasEntries()) stage->Run(*this, launch, dOut, n, outStride);
	}

	bool GpuBatch::StageHasEntries() const
	{
		for (const auto& stage : stages)
			if (stage && stage->HasEntries()) return true;
		return false;
	}

	// The stream leaves (ParkStream, RemoveStreams): a parked stream carries nothing over
	void GpuBatch::StageLeave(int s)
	{
		for (auto& stage : stages)
			if (stage) stage->Leave(s);
	}

	// test hooks (NA_DebugRunCabinetStage, NA_DebugRunCompressorStage, NA_DebugRunModStage, NA_DebugRunDelayStage, NA_DebugRunReverbStage, NA_DebugRunEqStage, NA_DebugRunMixStage): what a processing call of n samples runs for the stage, on host rows in
	// place of model outputs
	void GpuBatch::DebugRunStage(Stage& stage, const char* who, float* hostRows, long stride, size_t n, const float* hostIn)
	{
		if (!hostRows || n == 0 || stride < (long)n || streams.empty()) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": bad argument");
		Quiesce();
		if (!stage.HasEntries()) return;
		const size_t floats = (size_t)streams.size() * (size_t)stride;
		float *dRows = nullptr, *dIn = nullptr; // (hostIn: the input rows of the call, for a stage that reads them in front of the models)
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dRows), floats * sizeof(float)), "hipMalloc");
		try
		{
			if (hostIn)
			{
				CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dIn), floats * sizeof(float)), "hipMalloc");
				CheckHip(hipMemcpyAsync(dIn, hostIn, floats * sizeof(float), hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
			}
			CheckHip(hipMemcpyAsync(dRows, hostRows, floats * sizeof(float), hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
			stage.BeforeModels(*this, stream, dIn, n, stride);
			stage.Run(*this, stream, dRows, n, stride);
			CheckHip(hipMemcpyAsync(hostRows, dRows, floats * sizeof(float), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
			WaitStreamBounded(stream, "hipStreamSynchronize");
		}
		catch (...)
		{
			if (!broken)
			{
				(void)CountedHipFree(dRows);
				if (dIn) (void)CountedHipFree(dIn);
			}
			throw;
		}
		(void)CountedHipFree(dRows);
		if (dIn) (void)CountedHipFree(dIn);
	}

	// One choice per chunk (wavenet_choice.h WaveNetLaunchFor) and the launcher it names.  prepareOnly: upload the group tables the list's
	// launches will look up and launch nothing (the pass in front of a stream capture)
	void GpuBatch::LaunchWaveNetList(const ModelCall& c, LaunchKind which, const std::vector<WnFrameGroup>& list, hipStream_t s, bool prepareOnly)
	{
		WnLaunchTable& table = wnTable[(int)which];
		const bool frame = which == LaunchKind::Frame;
		const int sharing = 1 | WnBeyondCacheBit(StateBytes());
		const WnLaunchContext ctx = WnLaunchContext::Current();
		bool compact = false;
		for (const WnFrameGroup& g : list) compact = compact || g.model->compact_rings != 0;
		size_t offset = 0, left = c.n;
		while (left > 0)
		{
			const int chunk = NextWaveNetChunk(left, compact);
			const float* in = c.dIn + offset;
			float* out = c.dOut + offset;
			const WaveNetLaunchChoice choice = WaveNetLaunchChoiceOf(ctx, frame, list.data(), (int)list.size(), chunk, sharing, &wnFacts);
			if (choice.kernel == WnLaunchKernel::Pieces)
			{
				// more groups than one launch's kernarg table holds (a batch of many different models) and no table launch for them: launches
				// of eight groups each
				for (size_t first = 0; first < list.size() && !prepareOnly; first += WN_FRAME_MAX_GROUPS)
					CheckHip(LaunchWaveNetGroups(ctx, frame, list.data() + first, (int)std::min<size_t>(list.size() - first, (size_t)WN_FRAME_MAX_GROUPS), in, out, c.inStride,
						c.outStride, chunk, s, sharing), "WaveNet kernel (fused)");
			}
			else if (choice.kernel == WnLaunchKernel::ChainTable || !prepareOnly)
			{
				table.prepareOnly = prepareOnly;
				const hipError_t e = LaunchWaveNetChoice(choice, list.data(), (int)list.size(), in, out, c.inStride, c.outStride, chunk, s, &table);
				table.prepareOnly = false;
				CheckHip(e, choice.kernel == WnLaunchKernel::ChainTable ? "WaveNet kernel (table launch)" : "WaveNet kernel (fused)");
			}
			offset += (size_t)chunk;
			left -= (size_t)chunk;
		}
	}

	void GpuBatch::LaunchRecurrentUnit(const ModelCall& c, hipStream_t s, bool prepareOnly)
	{
		const std::vector<RecurrentGroup>& recArgs = c.recArgs;
		size_t offset = 0, left = c.n;
		while (left > 0)
		{
			const int chunk = (int)std::min<size_t>(left, (size_t)LSTM_MAX_FRAMES);
			if (recArgs.size() > (size_t)RECURRENT_MAX_GROUPS)
			{
				// (many different recurrent models: one launch, the group table in device memory)
				WnLaunchTable& table = wnTable[(int)LaunchKind::Recurrent];
				table.prepareOnly = prepareOnly;
				const hipError_t te = LaunchRecurrentDppTable(recArgs.data(), (int)recArgs.size(), c.dIn + offset, c.dOut + offset, c.inStride, c.outStride, chunk, s, table);
				table.prepareOnly = false;
				CheckHip(te, "RecurrentDppKernel (table launch)");
				offset += (size_t)chunk;
				left -= (size_t)chunk;
				continue;
			}
			if (prepareOnly) break;
			for (size_t first = 0; first < recArgs.size(); first += RECURRENT_MAX_GROUPS)
				CheckHip(LaunchRecurrentDpp(recArgs.data() + first, (int)std::min<size_t>(recArgs.size() - first, (size_t)RECURRENT_MAX_GROUPS),
					c.dIn + offset, c.dOut + offset, c.inStride, c.outStride, chunk, s), "RecurrentDppKernel (fused)");
			offset += (size_t)chunk;
			left -= (size_t)chunk;
		}
	}

	void GpuBatch::RunUnit(const ModelCall& c, size_t u, hipStream_t s, bool prepareOnly)
	{
		const LaunchUnit& unit = plan.units[u];
		if (unit.kind == LaunchKind::Recurrent) LaunchRecurrentUnit(c, s, prepareOnly);
		else if (unit.kind != LaunchKind::Own) LaunchWaveNetList(c, unit.kind, c.wnArgs[u], s, prepareOnly);
		else if (!prepareOnly) plan.groups[(size_t)unit.groups[0]]->Process(c.dIn, c.dOut, c.inStride, c.outStride, c.n, s);
	}

	// Several units: fork onto side streams so their kernels share the GPU, then join back into the batch stream.
	void GpuBatch::ForkJoinUnits(const ModelCall& c)
	{
		if (!forkEvent) CheckHip(CountedHipEventCreateWithFlags(&forkEvent, hipEventDisableTiming), "hipEventCreate");
		CheckHip(hipEventRecord(forkEvent, stream), "hipEventRecord");
		for (size_t u = 0; u < plan.units.size(); u++)
		{
			ModelGroup* owner = plan.groups[(size_t)plan.units[u].groups[0]];
			hipStream_t side = owner->SideStream();
			CheckHip(hipStreamWaitEvent(side, forkEvent, 0), "hipStreamWaitEvent");
			RunUnit(c, u, side, false);
			CheckHip(hipEventRecord(owner->DoneEvent(), side), "hipEventRecord");
			CheckHip(hipStreamWaitEvent(stream, owner->DoneEvent(), 0), "hipStreamWaitEvent");
		}
	}

	// The fork/join costs ~5 HIP calls per unit, which would make a buffer host-bound, so the sequence is captured once into a hipGraph
	// and replayed while the call signature (pointers, n, strides) and the active-stream lists stay the same -- the steady state of a
	// real-time host.
	void GpuBatch::ReplayUnitsGraph(const ModelCall& c)
	{
		hipGraphExec_t graphExec = nullptr;
		for (auto& e : graphCache)
			if (e.key.dIn == c.dIn && e.key.dOut == c.dOut && e.key.n == c.n && e.key.inStride == c.inStride && e.key.outStride == c.outStride) graphExec = e.exec;
		if (!graphExec)
		{
			if (graphCache.size() >= 16)
			{
				(void)hipGraphExecDestroy(graphCache.front().exec);
				graphCache.erase(graphCache.begin());
			}
			// the group tables of the table launches are uploaded here, in front of the capture (WnLaunchTable)
			for (size_t u = 0; u < plan.units.size(); u++) RunUnit(c, u, stream, true);
			hipGraph_t graph = nullptr;
			CheckHip(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed), "hipStreamBeginCapture");
			try
			{
				ForkJoinUnits(c);
			}
			catch (...)
			{
				(void)hipStreamEndCapture(stream, &graph);
				if (graph) (void)hipGraphDestroy(graph);
				throw;
			}
			CheckHip(hipStreamEndCapture(stream, &graph), "hipStreamEndCapture");
			const hipError_t e = hipGraphInstantiate(&graphExec, graph, nullptr, nullptr, 0);
			(void)hipGraphDestroy(graph);
			CheckHip(e, "hipGraphInstantiate");
			graphCache.push_back({ { c.dIn, c.dOut, c.n, c.inStride, c.outStride, topologyVersion }, graphExec });
		}
		CheckHip(hipGraphLaunch(graphExec, stream), "hipGraphLaunch");
	}

	// The model launches of a call, over n frames of device rows: one group's own launches, or the launch units of a mixed batch
	void GpuBatch::LaunchModelsOn(hipStream_t launch, const float* dIn, float* dOut, size_t n, long inStride, long outStride)
	{
		int activeGroups = 0;
		for (auto& g : groups) activeGroups += (g->NumActive() > 0);
		if (activeGroups <= 1)
		{
			for (auto& g : groups) g->Process(dIn, dOut, inStride, outStride, n, launch);
			return;
		}
		// Mixed batch: the launch units of launch_plan.h.  Their arguments are gathered first (changed index lists are uploaded now,
		// asynchronously on the batch stream: never inside a graph capture).
		UpdatePlan();
		const std::vector<LaunchUnit>& units = plan.units;
		ModelCall c{ dIn, dOut, n, inStride, outStride, std::vector<std::vector<WnFrameGroup>>(units.size()), {} };
		for (size_t u = 0; u < units.size(); u++)
		{
			if (units[u].kind == LaunchKind::Recurrent)
				for (int i : units[u].groups) c.recArgs.push_back(static_cast<LstmGroup*>(plan.groups[(size_t)i])->LaunchArgs());
			else if (units[u].kind == LaunchKind::Own) plan.groups[(size_t)units[u].groups[0]]->SyncActiveLists();
			else c.wnArgs[u] = WaveNetArgs(units[u], false);
		}
		// group tables of an earlier topology go (their graphs first)
		if (!graphCache.empty() && graphCache.front().key.version != topologyVersion)
		{
			for (auto& e : graphCache) (void)hipGraphExecDestroy(e.exec);
			graphCache.clear();
		}
		for (WnLaunchTable& t : wnTable) t.NewGeneration(topologyVersion);
		if (units.size() == 1)
		{
			RunUnit(c, 0, launch, false);
			return;
		}
		// tuning knob: the units one after the other on the batch stream instead of concurrently on side streams
		if (Tuning::Get().batchSerial)
		{
			for (size_t u = 0; u < units.size(); u++) RunUnit(c, u, stream, false);
			return;
		}
		// The runtime this process actually runs on may be OLDER than the ROCm 7.2 this library is built against: a host that loads
		// PyTorch first gets PyTorch's bundled libamdhip64 (HIP 7.0.51831 with torch 2.10+rocm7.0) for the whole process, and that
		// runtime's graph replay crashes after other graphs of the process were destroyed (hip::Graph::UpdateStreams under
		// hipGraphLaunch; seen in tests/test_gpu_multi.py behind any other test file, never on 7.2: profiles/r06_gputest_timing.txt).  On a
		// runtime older than the one it was built for the fork/join is therefore issued directly, every buffer: ~5 HIP calls per launch
		// unit of host time, the same streams, events and results.
		static const bool graphsTrusted = [] {
			int v = 0;
			return hipRuntimeGetVersion(&v) == hipSuccess && v >= 70200000 && !Tuning::Get().batchNoGraph;
		}();
		if (graphsTrusted) ReplayUnitsGraph(c);
		else ForkJoinUnits(c);
	}

	void GpuBatch::WeightImages(const LoadedModel& model, std::vector<std::pair<void*, size_t>>& out) const
	{
		for (const auto& sub : model.subModels)
			for (const auto& g : groups)
				if (g->desc.get() == sub.desc.get()) g->WeightImages(out);
	}

	void GpuBatch::WeightsArrived()
	{
		CheckUsable();
		CheckHip(hipSetDevice(device), "hipSetDevice");
		for (ModelGroup* g : awaitingWeights) g->WeightsArrived();
		awaitingWeights.clear();
		for (auto& pp : pendingPrewarm) pp.first->Prewarm(pp.second);
		pendingPrewarm.clear();
		peerWeights = false;
	}

	void GpuBatch::Synchronize()
	{
		Quiesce();
	}

	double GpuBatch::AlgorithmicBytesPerSample(int blockFrames) const
	{
		double sum = 0.0;
		int n = 0;
		for (const auto& g : groups)
		{
			sum += g->AlgorithmicBytesPerSample(blockFrames) * g->NumActive();
			n += g->NumActive();
		}
		return n ? sum / n : 0.0;
	}

	double GpuBatch::MacsPerSample() const
	{
		double sum = 0.0;
		int n = 0;
		for (const auto& g : groups)
		{
			sum += g->MacsPerSample() * g->NumActive();
			n += g->NumActive();
		}
		return n ? sum / n : 0.0;
	}

	const char* GpuBatch::StreamKernelName(int s) const
	{
		const StreamRef& ref = streams.at((size_t)s);
		if (!ref.live) return "";
		return ref.members[(size_t)ref.active].first->KernelName();
	}

	float GpuBatch::StreamInputLimit(int s) const
	{
		const StreamRef& ref = streams.at((size_t)s);
		if (!ref.live) return 0.0f;
		return ref.members[(size_t)ref.active].first->InputLimit();
	}

	int GpuBatch::StreamRangeEvents(int s)
	{
		CheckUsable();
		const StreamRef& ref = streams.at((size_t)s);
		if (!ref.live) return 0;
		CheckHip(hipSetDevice(device), "hipSetDevice");
		DrainPipeline();
		int total = 0;
		for (const auto& gm : ref.members) total += gm.first->RangeEvents(gm.second);
		return total;
	}

	int GpuBatch::StreamPackFactor(int s) const
	{
		const StreamRef& ref = streams.at((size_t)s);
		if (!ref.live) return 0;
		return ref.members[(size_t)ref.active].first->PackFactor();
	}

	size_t GpuBatch::StateBytes() const
	{
		size_t total = 0;
		for (const auto& g : groups) total += g->StateBytesPerStream() * (size_t)g->NumInUse();
		return total;
	}
}
