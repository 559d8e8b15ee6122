// stream_snapshot.h -- the relocatable snapshot of one stream's state: what NA_BatchSaveStreams writes and
// NA_BatchLoadStreams reads.  Host-side definition only: sizes, header, fingerprint; the device kernels that gather a stream out of
// its state layout and scatter it back are in stream_snapshot_kernels.hip.
//
// One blob per stream, little-endian, every field and every value 32 bits wide (two 64-bit fields are 8-byte aligned):
//
//     offset  field
//          0  u32 magic          'N' 'A' 'S' 'S'
//          4  u32 version        kSnapshotVersion
//          8  u64 totalBytes     the whole blob
//         16  u64 fingerprint    ModelFingerprint(): architecture + flat weights of every submodel
//         24  u32 numSubModels
//         28  u32 activeSubModel
//         32  f32 quality
//         36  u32 flags          bit 0: the source stream's load mode was OnDemand
//         40  u32 prewarmedMask  bit k: submodel k had its initial prewarm
//         44  u32 headerBytes    offset of the first section's payload = 48 + 16 numSubModels
//         48  section table, 16 bytes per submodel: u32 kind (ModelKind), u32 encoding, u32 values, u32 offset (bytes from the blob start)
//     payload of section 0, section 1, ... back to back, `values` 32-bit words each
//
// WaveNet section: per ring of the plan, in plan order (the layers of every array, then the array's conv-head ring if it has one),
// the last (K - 1) d frames of that layer's input, oldest frame first, a frame = its real channels.  Recurrent section: the state rows
// as LstmGroup orders them (h / c per layer, then the conv1d history rows of the tail).  Ring cursors and the range-event counter are
// not part of a snapshot.
//
// Encoding of a section's values: SNAP_F32 = IEEE f32; SNAP_SPLIT = the f16-split kernels' native pair as h | l << 16 (h = f16(v),
// l = f16(v - h)).  A split value is NOT normalised to f32 on save: h + l is exact in f32, but splitting the sum again may return
// another pair with the same sum (v just inside a rounding tie of h), and the three-product split arithmetic is not invariant under that.
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "model_loader.h"

namespace na
{
	constexpr uint32_t kSnapshotMagic = 0x5353414Eu; // "NASS"
	constexpr uint32_t kSnapshotVersion = 1;
	constexpr size_t kSnapshotFixedHeaderBytes = 48;
	constexpr size_t kSnapshotSectionEntryBytes = 16;
	enum SnapshotEncoding : uint32_t { SNAP_F32 = 0, SNAP_SPLIT = 1 };

	struct SnapshotSection
	{
		uint32_t kind, encoding, values, offset;
	};

	struct SnapshotHeader
	{
		uint32_t magic, version;
		uint64_t totalBytes, fingerprint;
		uint32_t numSubModels, activeSubModel;
		float quality;
		uint32_t flags, prewarmedMask, headerBytes;
	};
	static_assert(sizeof(SnapshotHeader) == kSnapshotFixedHeaderBytes, "the snapshot header is 48 bytes");
	static_assert(sizeof(SnapshotSection) == kSnapshotSectionEntryBytes, "a section entry is 16 bytes");

	// one ring of a WaveNet section: `history` frames of `channels` values
	struct SnapshotRing
	{
		int history, channels;
	};

	// the rings of a WaveNet in plan order (wavenet_plan.cpp: AddRing per layer, then the conv-head ring of the array)
	inline std::vector<SnapshotRing> SnapshotRings(const WaveNetDesc& wn)
	{
		std::vector<SnapshotRing> rings;
		for (const WnArrayCfg& cfg : wn.arrays)
		{
			for (size_t l = 0; l < cfg.kernelSizes.size(); l++) rings.push_back({ (cfg.kernelSizes[l] - 1) * cfg.dilations[l], cfg.channels });
			if (cfg.headKernelSize > 1) rings.push_back({ (cfg.headKernelSize - 1) * cfg.headDilation, cfg.channels });
		}
		return rings;
	}

	// 32-bit values in the section of one submodel
	inline size_t SnapshotSectionValues(const ModelDesc& d)
	{
		size_t n = 0;
		if (d.kind == MODEL_WAVENET)
		{
			for (const SnapshotRing& r : SnapshotRings(d.wavenet)) n += (size_t)r.history * (size_t)r.channels;
		}
		else if (d.kind == MODEL_LSTM)
		{
			n = (size_t)d.lstm.numLayers * 2 * (size_t)d.lstm.hiddenSize;
			for (const DenseLayerDesc& dl : d.lstm.tail) n += (size_t)dl.History() * (size_t)dl.in;
		}
		return n;
	}

	inline size_t SnapshotHeaderBytes(const LoadedModel& m) { return kSnapshotFixedHeaderBytes + kSnapshotSectionEntryBytes * m.subModels.size(); }

	inline size_t SnapshotBytes(const LoadedModel& m)
	{
		size_t n = SnapshotHeaderBytes(m);
		for (const SubModel& s : m.subModels) n += 4 * SnapshotSectionValues(*s.desc);
		return n;
	}

	// FNV-1a (64 bit) over the architecture description and the flat weights of every submodel, as the loader produced them (ModelDesc):
	// nothing of a kernel's weight image, no math mode, no tuning knob -- the same file gives the same number in every batch, device,
	// process and kernel family
	class SnapshotHash
	{
	public:
		void Int(long long v) { Bytes(&v, sizeof v); }
		void Floats(const std::vector<float>& v)
		{
			Int((long long)v.size());
			if (!v.empty()) Bytes(v.data(), v.size() * sizeof(float));
		}
		void Ints(const std::vector<int>& v)
		{
			Int((long long)v.size());
			for (int x : v) Int(x);
		}
		uint64_t Value() const { return h; }

	private:
		void Bytes(const void* p, size_t n)
		{
			const unsigned char* b = static_cast<const unsigned char*>(p);
			for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
		}
		uint64_t h = 0xCBF29CE484222325ull;
	};

	inline uint64_t ModelFingerprint(const LoadedModel& m)
	{
		SnapshotHash f;
		f.Int((long long)m.subModels.size());
		for (const SubModel& s : m.subModels)
		{
			const ModelDesc& d = *s.desc;
			f.Int(d.kind);
			if (d.kind == MODEL_WAVENET)
			{
				f.Int((long long)d.wavenet.arrays.size());
				for (const WnArrayCfg& c : d.wavenet.arrays)
				{
					for (int v : { c.inputSize, c.conditionSize, c.headSize, c.headKernelSize, c.headDilation, c.channels, c.hasHeadBias ? 1 : 0, c.activation }) f.Int(v);
					f.Ints(c.kernelSizes);
					f.Ints(c.dilations);
				}
				f.Floats(d.wavenet.weights);
			}
			else if (d.kind == MODEL_LSTM)
			{
				for (int v : { d.lstm.cell, d.lstm.numLayers, d.lstm.hiddenSize }) f.Int(v);
				for (const LSTMLayerDesc& l : d.lstm.layers)
				{
					f.Int(l.inputSize);
					f.Floats(l.w);
					f.Floats(l.bias);
					f.Floats(l.h0);
					f.Floats(l.c0);
				}
				f.Floats(d.lstm.headWeights);
				f.Floats({ d.lstm.headBias });
				f.Int((long long)d.lstm.tail.size());
				for (const DenseLayerDesc& t : d.lstm.tail)
				{
					for (int v : { t.in, t.out, t.activation, t.ksize, t.dilation }) f.Int(v);
					f.Floats(t.w);
					f.Floats(t.b);
				}
			}
		}
		return f.Value();
	}

	// Host-side check of one blob against the model of the stream it is meant for; throws std::runtime_error naming the reason.
	// `available`: bytes from the blob's start to the end of the caller's buffer.  Returns the blob's size.
	inline size_t ValidateSnapshot(const void* blob, size_t available, const LoadedModel& model, uint64_t fingerprint, const std::string& who)
	{
		auto fail = [&](const std::string& why) -> size_t { throw std::runtime_error(who + ": " + why); };
		if (available < kSnapshotFixedHeaderBytes) return fail("truncated snapshot (shorter than its header)");
		SnapshotHeader h;
		memcpy(&h, blob, sizeof h);
		if (h.magic != kSnapshotMagic) return fail("bad magic word (not a stream snapshot)");
		if (h.version != kSnapshotVersion) return fail("unsupported snapshot version " + std::to_string(h.version) + " (this library reads version " + std::to_string(kSnapshotVersion) + ")");
		if (h.totalBytes > available) return fail("truncated snapshot (" + std::to_string(available) + " bytes of " + std::to_string(h.totalBytes) + ")");
		if (h.fingerprint != fingerprint) return fail("model fingerprint mismatch (the snapshot was taken from another model)");
		if (h.numSubModels != model.subModels.size()) return fail("submodel count mismatch");
		if (h.totalBytes != SnapshotBytes(model) || h.headerBytes != SnapshotHeaderBytes(model)) return fail("snapshot size does not match the model");
		if (h.activeSubModel >= h.numSubModels) return fail("active submodel out of range");
		size_t offset = h.headerBytes;
		for (size_t k = 0; k < model.subModels.size(); k++)
		{
			SnapshotSection s;
			memcpy(&s, static_cast<const char*>(blob) + kSnapshotFixedHeaderBytes + k * kSnapshotSectionEntryBytes, sizeof s);
			const ModelDesc& d = *model.subModels[k].desc;
			if (s.kind != (uint32_t)d.kind || s.values != SnapshotSectionValues(d) || s.offset != offset) return fail("section table does not match the model");
			if (s.encoding != SNAP_F32 && !(s.encoding == SNAP_SPLIT && d.kind == MODEL_WAVENET)) return fail("unknown section encoding");
			offset += 4 * (size_t)s.values;
		}
		return (size_t)h.totalBytes;
	}

	// ---- device side (stream_snapshot_kernels.hip) ----------------------------------------------------------------------------------
	// One launch serves every listed stream of a model group.  `lists` = [slot | sub | encoding] x count ints: the state slot (of the
	// virtual stream in a packed group), the stream's position inside a pack, the encoding of its section in the staging buffer (import).
	// `snapTab` = 4 ints per ring: history frames, real channels, virtual channels a stream owns (the whole ring when unpacked), word
	// offset of the ring inside a section.  Sections sit back to back in `staging`, `sectionWords` apart, in list order.
	struct WnSnapshotArgs
	{
		float* state;
		int stateF4;
		const int* lists;
		int count, numRings;
		const int *ringOffF4, *ringFrames, *ringG, *snapTab;
		int split; // the state format: 1 = split quads, frame-major rings; 0 = f32 quads in the tile layout
		int pack;
		int sectionWords;
	};
	hipError_t LaunchWaveNetSnapshotExport(const WnSnapshotArgs& a, uint32_t* staging, hipStream_t stream);
	hipError_t LaunchWaveNetSnapshotImport(const WnSnapshotArgs& a, const uint32_t* staging, hipStream_t stream);
	// SoA recurrent state[row * capacity + slot] <-> staging[i * numElems + row] for the listed slots
	hipError_t LaunchRecurrentSnapshot(float* state, int capacity, const int* slots, int count, int numElems, uint32_t* staging, bool import, hipStream_t stream);
	long long SnapshotKernelLaunches(); // export / import launches so far (test hook NA_DebugSnapshotLaunches)
}
