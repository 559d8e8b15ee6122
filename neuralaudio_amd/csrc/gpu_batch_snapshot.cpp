// gpu_batch_snapshot.cpp -- save and restore of live stream state (gpu_batch.h SaveStreams / LoadStreams; format: stream_snapshot.h,
// kernels: stream_snapshot_kernels.hip).  The reference has no counterpart: its unit of state is a C++ object in the host's address
// space (one InternalWaveNetModelT / InternalLSTMModelT per stream, NeuralAudio/InternalModel.h:84-160, 300-372); here the state sits
// in device memory in the layouts of four kernel families, and a snapshot is the layout-independent form of it.
#include "gpu_batch_internal.h"

#include <map>

namespace na
{
	namespace
	{
		// the sections of one call, grouped by model group: every group's members get one contiguous region of the staging buffer
		struct GroupPart
		{
			std::vector<int> members;
			std::vector<uint32_t> encodings;               // LoadStreams: of each member's section
			std::vector<std::pair<int, int>> origin;        // (index into ids, submodel) of each member
			size_t firstWord = 0;
		};
	}

	uint64_t GpuBatch::FingerprintOf(const std::shared_ptr<const LoadedModel>& model)
	{
		for (const auto& f : fingerprints)
			if (f.first.get() == model.get()) return f.second;
		fingerprints.push_back({ model, ModelFingerprint(*model) });
		return fingerprints.back().second;
	}

	void GpuBatch::EnsureSnapshotStaging(size_t words)
	{
		if (words <= snapWords) return;
		if (snapHost) (void)CountedHipHostFree(snapHost);
		if (snapDev) (void)CountedHipFree(snapDev);
		snapHost = nullptr;
		snapDev = nullptr;
		snapWords = 0;
		CheckHip(CountedHipHostMalloc(reinterpret_cast<void**>(&snapHost), words * sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc");
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&snapDev), words * sizeof(uint32_t)), "hipMalloc");
		snapWords = words;
	}

	size_t GpuBatch::StreamSnapshotBytes(int s) const
	{
		if (IsParked(s)) throw std::runtime_error("neuralaudio_amd: StreamSnapshotBytes: stream " + std::to_string(s) + " is parked");
		if (!IsLive(s)) throw std::runtime_error("neuralaudio_amd: StreamSnapshotBytes: no such stream");
		return SnapshotBytes(*streams[(size_t)s].model);
	}

	// what RemoveStreams does before it touches state: nothing of the batch is in flight any more, no prewarm is pending
	void GpuBatch::SettleForSnapshot(const int* ids, int count, const char* who)
	{
		CheckUsable();
		// (the v1 blob has no place for the resampler's histories, and the phase is the batch's, not the stream's)
		if (Resamples()) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": stream snapshots of a resampling batch are not supported");
		if (count < 0 || (count > 0 && !ids)) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": bad argument");
		for (int i = 0; i < count; i++)
			if (IsParked(ids[i])) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": stream " + std::to_string(ids[i]) + " is parked (a parked stream has no state of its own: it is armed)");
		for (int i = 0; i < count; i++)
			if (!IsLive(ids[i])) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": stream " + std::to_string(ids[i]) + " is not a live stream of the batch");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		// (deferred prewarms exist only while weights are awaited and run in WeightsArrived: past this check none is pending, so a
		// stream saved right after AddStreams(doPrewarm = 1) holds its prewarmed state)
		if (AwaitsWeights()) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": the batch still waits for a peer device's weights (WeightsArrived)");
		Quiesce();
	}

	size_t GpuBatch::SaveStreams(const int* ids, int count, void* buf, size_t capacity)
	{
		SettleForSnapshot(ids, count, "SaveStreams");
		size_t total = 0;
		for (int i = 0; i < count; i++) total += SnapshotBytes(*streams[(size_t)ids[i]].model);
		if (total > capacity || count == 0) return total;
		if (!buf) throw std::runtime_error("neuralaudio_amd: SaveStreams: null buffer");

		std::map<ModelGroup*, GroupPart> parts;
		std::vector<ModelGroup*> order; // first use, so that the staging layout does not depend on pointer values
		for (int i = 0; i < count; i++)
		{
			const StreamRef& ref = streams[(size_t)ids[i]];
			for (size_t k = 0; k < ref.members.size(); k++)
			{
				ModelGroup* g = ref.members[k].first;
				if (!parts.count(g)) order.push_back(g);
				GroupPart& p = parts[g];
				p.members.push_back(ref.members[k].second);
				p.origin.push_back({ i, (int)k });
			}
		}
		size_t words = 0;
		for (ModelGroup* g : order)
		{
			parts[g].firstWord = words;
			words += parts[g].members.size() * g->SnapshotValues();
		}
		EnsureSnapshotStaging(std::max<size_t>(words, 1));
		for (ModelGroup* g : order) g->SaveState(parts[g].members, snapDev + parts[g].firstWord); // one launch per group
		if (words) CheckHip(hipMemcpyAsync(snapHost, snapDev, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync D2H");
		WaitStreamBounded(stream, "SaveStreams");

		// where section k of stream i landed
		std::vector<std::vector<const uint32_t*>> section((size_t)count);
		for (int i = 0; i < count; i++) section[(size_t)i].resize(streams[(size_t)ids[i]].members.size());
		for (ModelGroup* g : order)
		{
			const GroupPart& p = parts[g];
			for (size_t j = 0; j < p.members.size(); j++)
				section[(size_t)p.origin[j].first][(size_t)p.origin[j].second] = snapHost + p.firstWord + j * g->SnapshotValues();
		}
		char* out = static_cast<char*>(buf);
		for (int i = 0; i < count; i++)
		{
			const StreamRef& ref = streams[(size_t)ids[i]];
			SnapshotHeader h = {};
			h.magic = kSnapshotMagic;
			h.version = kSnapshotVersion;
			h.totalBytes = SnapshotBytes(*ref.model);
			h.fingerprint = FingerprintOf(ref.model);
			h.numSubModels = (uint32_t)ref.members.size();
			h.activeSubModel = (uint32_t)ref.active;
			h.quality = ref.quality;
			h.flags = ref.onDemand ? 1u : 0u;
			h.prewarmedMask = StreamPrewarmedMask(ids[i]);
			h.headerBytes = (uint32_t)SnapshotHeaderBytes(*ref.model);
			memcpy(out, &h, sizeof h);
			size_t offset = h.headerBytes;
			for (size_t k = 0; k < ref.members.size(); k++)
			{
				ModelGroup* g = ref.members[k].first;
				const SnapshotSection s = { (uint32_t)g->desc->kind, g->SnapshotNativeEncoding(), (uint32_t)g->SnapshotValues(), (uint32_t)offset };
				memcpy(out + kSnapshotFixedHeaderBytes + k * kSnapshotSectionEntryBytes, &s, sizeof s);
				memcpy(out + offset, section[(size_t)i][k], 4 * (size_t)s.values);
				offset += 4 * (size_t)s.values;
			}
			out += h.totalBytes;
		}
		return total;
	}

	void GpuBatch::LoadStreams(const int* ids, int count, const void* buf, size_t bytes)
	{
		SettleForSnapshot(ids, count, "LoadStreams");
		if (count == 0) return;
		if (!buf) throw std::runtime_error("neuralaudio_amd: LoadStreams: null buffer");
		// ---- every check before the first write
		{
			std::vector<int> sorted(ids, ids + count);
			std::sort(sorted.begin(), sorted.end());
			if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) throw std::runtime_error("neuralaudio_amd: LoadStreams: a stream is named twice");
		}
		std::vector<const char*> blob((size_t)count);
		const char* at = static_cast<const char*>(buf);
		size_t left = bytes;
		for (int i = 0; i < count; i++)
		{
			const StreamRef& ref = streams[(size_t)ids[i]];
			const size_t n = ValidateSnapshot(at, left, *ref.model, FingerprintOf(ref.model),
				"neuralaudio_amd: LoadStreams: snapshot " + std::to_string(i) + " (for stream " + std::to_string(ids[i]) + ")");
			blob[(size_t)i] = at;
			at += n;
			left -= n;
		}

		// ---- sections -> pinned staging, grouped by model group
		std::map<ModelGroup*, GroupPart> parts;
		std::vector<ModelGroup*> order;
		for (int i = 0; i < count; i++)
		{
			const StreamRef& ref = streams[(size_t)ids[i]];
			for (size_t k = 0; k < ref.members.size(); k++)
			{
				ModelGroup* g = ref.members[k].first;
				if (!parts.count(g)) order.push_back(g);
				GroupPart& p = parts[g];
				SnapshotSection s;
				memcpy(&s, blob[(size_t)i] + kSnapshotFixedHeaderBytes + k * kSnapshotSectionEntryBytes, sizeof s);
				p.members.push_back(ref.members[k].second);
				p.encodings.push_back(s.encoding);
				p.origin.push_back({ i, (int)k });
			}
		}
		size_t words = 0;
		for (ModelGroup* g : order)
		{
			parts[g].firstWord = words;
			words += parts[g].members.size() * g->SnapshotValues();
		}
		EnsureSnapshotStaging(std::max<size_t>(words, 1));
		for (ModelGroup* g : order)
		{
			const GroupPart& p = parts[g];
			for (size_t j = 0; j < p.members.size(); j++)
			{
				SnapshotSection s;
				memcpy(&s, blob[(size_t)p.origin[j].first] + kSnapshotFixedHeaderBytes + (size_t)p.origin[j].second * kSnapshotSectionEntryBytes, sizeof s);
				memcpy(snapHost + p.firstWord + j * g->SnapshotValues(), blob[(size_t)p.origin[j].first] + s.offset, 4 * (size_t)s.values);
			}
		}

		// ---- quality and active submodel through SetQuality's own path (active lists, launch plan); a switch may prewarm an OnDemand
		// destination's submodel -- the import below overwrites that state, the bits of the source follow after it
		for (int i = 0; i < count; i++)
		{
			SnapshotHeader h;
			memcpy(&h, blob[(size_t)i], sizeof h);
			SetQuality(ids[i], h.quality);
			StreamRef& ref = streams[(size_t)ids[i]];
			if (ref.active != (int)h.activeSubModel)
			{
				// (the same file maps a quality to the same submodel; a blob that says otherwise is followed to the letter)
				ref.members[(size_t)ref.active].first->SetActive(ref.members[(size_t)ref.active].second, -1);
				ref.active = (int)h.activeSubModel;
				ref.members[(size_t)ref.active].first->SetActive(ref.members[(size_t)ref.active].second, ids[i]);
				topologyVersion++;
			}
		}
		Quiesce(); // (a prewarm inside SetQuality ran on the batch stream)
		if (words) CheckHip(hipMemcpyAsync(snapDev, snapHost, words * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "hipMemcpyAsync H2D");
		for (ModelGroup* g : order) g->LoadState(parts[g].members, parts[g].encodings, snapDev + parts[g].firstWord); // one launch per group
		WaitStreamBounded(stream, "LoadStreams");
		for (int i = 0; i < count; i++)
		{
			SnapshotHeader h;
			memcpy(&h, blob[(size_t)i], sizeof h);
			StreamRef& ref = streams[(size_t)ids[i]];
			for (size_t k = 0; k < ref.prewarmed.size(); k++) ref.prewarmed[k] = (k < 32 && ((h.prewarmedMask >> k) & 1u)) ? 1 : 0;
		}
	}
}
