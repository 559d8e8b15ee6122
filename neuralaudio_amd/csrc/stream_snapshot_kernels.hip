// stream_snapshot_kernels.hip -- gather a stream's state out of its layout into the canonical snapshot section (stream_snapshot.h:
// [ring][frame][channel] words, oldest frame first, real channels only) and scatter it back, for every stream-state format:
//   f16-split kernels: split quads [h0 h1 | h2 h3 | l0 l1 | l2 l3], frame-major rings (quad of channel group g of position p: p * G + g)
//   frame / runtime-shaped kernels: f32 quads in the tile layout (quad index (p >> 4) * G * 16 + g * 16 + (p & 15))
//   roomy, exact and compact rings alike: every one is a true modulo ring, and between two launches the frame t samples back sits at
//   position (cursor - t) mod R for every t up to the layer's history (a kept frame is addressed from the cursor AFTER its block)
//   packed virtual streams: stream `sub` owns the virtual channels [sub * Cp, (sub + 1) * Cp) of a ring, Cp = ring channels / pack --
//   whole channel groups, or in a dense pack (Cp == 2) one half of a quad: dwords (sub & 1) and 2 + (sub & 1)
//   padded models: the real channels are the first ones of what the stream owns; the rest is written as zeros, never exported
// The processing kernels are untouched: these read and write the state between launches (the host has quiesced the batch).
#include <atomic>

#include <hip/hip_runtime.h>

#include "stream_snapshot.h"
#include "wavenet_dev.h"

namespace na
{
	namespace
	{
		typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

		// value k of a split quad as the snapshot word h | l << 16
		__device__ __forceinline__ unsigned SplitWord(const u32x4 q, int k)
		{
			const unsigned hw = (k & 2) ? q.y : q.x, lw = (k & 2) ? q.w : q.z;
			const unsigned sh = (k & 1) ? 16u : 0u;
			return ((hw >> sh) & 0xFFFFu) | (((lw >> sh) & 0xFFFFu) << 16);
		}

		__device__ __forceinline__ unsigned F16Bits(_Float16 h) { return (unsigned)__builtin_bit_cast(unsigned short, h); }

		// one snapshot word -> the destination format's 32 bits: a split pair (h | l << 16) or an f32
		__device__ __forceinline__ unsigned ConvertWord(unsigned w, int srcEnc, int dstSplit)
		{
			if (dstSplit)
			{
				if (srcEnc == (int)SNAP_SPLIT) return w; // bit for bit
				// f32 -> split, as SplitQuadBits does (wavenet_prewarm_kernels.hip): h = f16(v), l = f16(v - h)
				const float v = __builtin_bit_cast(float, w);
				const _Float16 h = (_Float16)v;
				const _Float16 l = (_Float16)(v - (float)h);
				return F16Bits(h) | (F16Bits(l) << 16);
			}
			if (srcEnc == (int)SNAP_F32) return w;
			// split -> f32: h + l is exact in f32
			const float h = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu));
			const float l = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
			return __builtin_bit_cast(unsigned, h + l);
		}

		// what thread item `idx` of ring r works on: frame t of the history (oldest = 0) and channel group g of the ring; false: nothing.
		// Split format: consecutive items walk the owned channel groups of one frame, then the next frame (a wave of an unpacked stream
		// touches 1 KB of consecutive quads); tile layout: sixteen consecutive frames of one channel group (a 256-byte row), then the next group.
		struct RingGeo
		{
			int R, G, hist, C, owned, wordOff, g0, og, items;
		};

		__device__ __forceinline__ RingGeo Geometry(const int* ringFrames, const int* ringG, const int* snapTab, int r, int sub, int pack)
		{
			RingGeo q;
			q.R = ringFrames[r];
			q.G = ringG[r];
			q.hist = snapTab[4 * r];
			q.C = snapTab[4 * r + 1];
			q.owned = snapTab[4 * r + 2];
			q.wordOff = snapTab[4 * r + 3];
			q.g0 = pack > 1 ? (sub * q.owned) >> 2 : 0;       // first channel group the stream owns (dense pack: the one it shares)
			q.og = q.owned >= 4 ? q.owned >> 2 : 1;            // channel groups it touches
			q.items = ((q.hist + 15) & ~15) * q.og;
			return q;
		}

		__device__ __forceinline__ bool Item(const RingGeo& q, int idx, int split, int& t, int& g)
		{
			int gi;
			if (split)
			{
				t = idx / q.og;
				gi = idx - t * q.og;
			}
			else
			{
				const int row = idx >> 4;
				const int tile = row / q.og;
				gi = row - tile * q.og;
				t = tile * 16 + (idx & 15);
			}
			g = q.g0 + gi;
			return t < q.hist && g < q.G;
		}

		// quad index (16-byte units from the ring start) of channel group g at `back` = hist - t frames behind the cursor
		__device__ __forceinline__ int QuadIndex(const RingGeo& q, int cursor, int t, int g, int split)
		{
			int p = cursor - (q.hist - t); // hist <= R: one wrap
			if (p < 0) p += q.R;
			return split ? p * q.G + g : (p >> 4) * q.G * 16 + g * 16 + (p & 15);
		}

		// grid = (streams of the call, rings), block = 256
		__global__ void __launch_bounds__(256) WaveNetSnapshotExportKernel(const u32x4* __restrict__ state, int stateF4, const int* __restrict__ lists, int count,
			const int* __restrict__ ringOffF4, const int* __restrict__ ringFrames, const int* __restrict__ ringG, const int* __restrict__ snapTab, int split, int pack,
			int sectionWords, unsigned* __restrict__ staging)
		{
			const int i = blockIdx.x, r = blockIdx.y;
			const int slot = lists[i], sub = pack > 1 ? lists[count + i] : 0;
			const u32x4* st = state + (size_t)slot * (size_t)stateF4;
			const RingGeo q = Geometry(ringFrames, ringG, snapTab, r, sub, pack);
			if (q.hist == 0) return;
			int cursor = reinterpret_cast<const int*>(st)[r];
			if (cursor < 0 || cursor >= q.R) cursor = 0; // (never so in a stream the library set up; keeps every address inside the ring)
			const u32x4* ring = st + ringOffF4[r];
			unsigned* out = staging + (size_t)i * (size_t)sectionWords + q.wordOff;
			const int c0 = sub * q.owned; // first virtual channel of the stream
			for (int idx = threadIdx.x; idx < q.items; idx += blockDim.x)
			{
				int t, g;
				if (!Item(q, idx, split, t, g)) continue;
				const u32x4 v = ring[QuadIndex(q, cursor, t, g, split)];
#pragma unroll
				for (int k = 0; k < 4; k++)
				{
					const int c = 4 * g + k - c0;
					if (c < 0 || c >= q.C || c >= q.owned) continue;
					out[t * q.C + c] = split ? SplitWord(v, k) : (k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)));
				}
			}
		}

		// The inverse.  Cursors are left where they stand (in a packed virtual stream they belong to running neighbours too): the frames
		// go to the positions the destination's cursor implies.  Channels the stream owns beyond the real ones are written as zeros; in a
		// dense pack the stream's two dwords of a shared quad are stored one by one (the other two belong to a stream that another
		// workgroup of this launch may be filling); everything else of the state is untouched.
		__global__ void __launch_bounds__(256) WaveNetSnapshotImportKernel(u32x4* __restrict__ state, int stateF4, const int* __restrict__ lists, int count,
			const int* __restrict__ ringOffF4, const int* __restrict__ ringFrames, const int* __restrict__ ringG, const int* __restrict__ snapTab, int split, int pack,
			int sectionWords, const unsigned* __restrict__ staging)
		{
			const int i = blockIdx.x, r = blockIdx.y;
			const int slot = lists[i], sub = pack > 1 ? lists[count + i] : 0, enc = lists[2 * count + i];
			u32x4* st = state + (size_t)slot * (size_t)stateF4;
			const RingGeo q = Geometry(ringFrames, ringG, snapTab, r, sub, pack);
			if (q.hist == 0) return;
			int cursor = reinterpret_cast<const int*>(st)[r];
			if (cursor < 0 || cursor >= q.R) cursor = 0;
			u32x4* ring = st + ringOffF4[r];
			const unsigned* in = staging + (size_t)i * (size_t)sectionWords + q.wordOff;
			const int c0 = sub * q.owned;
			const bool halfQuad = q.owned < 4; // dense pack
			for (int idx = threadIdx.x; idx < q.items; idx += blockDim.x)
			{
				int t, g;
				if (!Item(q, idx, split, t, g)) continue;
				unsigned w[4];
#pragma unroll
				for (int k = 0; k < 4; k++)
				{
					const int c = 4 * g + k - c0;
					const bool real = c >= 0 && c < q.C && c < q.owned;
					w[k] = real ? ConvertWord(in[t * q.C + c], enc, split) : 0u; // (zero is zero in both formats)
				}
				u32x4 v;
				if (split)
				{
					v.x = (w[0] & 0xFFFFu) | (w[1] << 16);
					v.y = (w[2] & 0xFFFFu) | (w[3] << 16);
					v.z = (w[0] >> 16) | (w[1] & 0xFFFF0000u);
					v.w = (w[2] >> 16) | (w[3] & 0xFFFF0000u);
				}
				else v = u32x4{ w[0], w[1], w[2], w[3] };
				const int qi = QuadIndex(q, cursor, t, g, split);
				if (halfQuad)
				{
					const int half = sub & 1;
					unsigned* d = reinterpret_cast<unsigned*>(ring + qi);
					d[half] = half ? v.y : v.x;
					d[2 + half] = half ? v.w : v.z;
				}
				else ring[qi] = v;
			}
		}

		// grid = (ceil(count / 256), numElems): thread = stream, so that the state side (row-major over slots) is the coalesced one
		__global__ void __launch_bounds__(256) RecurrentSnapshotKernel(float* __restrict__ state, int capacity, const int* __restrict__ slots, int count, int numElems,
			unsigned* __restrict__ staging, int import)
		{
			const int i = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
			if (i >= count) return;
			const int slot = slots[i];
			if (slot < 0 || slot >= capacity) return;
			float* s = state + (size_t)e * (size_t)capacity + slot;
			unsigned* w = staging + (size_t)i * (size_t)numElems + e;
			if (import) *s = __builtin_bit_cast(float, *w);
			else *w = __builtin_bit_cast(unsigned, *s);
		}

		std::atomic<long long> g_snapshotLaunches{ 0 };
	}

	long long SnapshotKernelLaunches() { return g_snapshotLaunches.load(); }

	hipError_t LaunchWaveNetSnapshotExport(const WnSnapshotArgs& a, uint32_t* staging, hipStream_t stream)
	{
		if (a.count <= 0 || a.numRings <= 0) return hipSuccess;
		g_snapshotLaunches++;
		hipLaunchKernelGGL(WaveNetSnapshotExportKernel, dim3((unsigned)a.count, (unsigned)a.numRings), dim3(256), 0, stream,
			reinterpret_cast<const u32x4*>(a.state), a.stateF4, a.lists, a.count, a.ringOffF4, a.ringFrames, a.ringG, a.snapTab, a.split, a.pack, a.sectionWords, staging);
		return hipGetLastError();
	}

	hipError_t LaunchWaveNetSnapshotImport(const WnSnapshotArgs& a, const uint32_t* staging, hipStream_t stream)
	{
		if (a.count <= 0 || a.numRings <= 0) return hipSuccess;
		g_snapshotLaunches++;
		hipLaunchKernelGGL(WaveNetSnapshotImportKernel, dim3((unsigned)a.count, (unsigned)a.numRings), dim3(256), 0, stream,
			reinterpret_cast<u32x4*>(a.state), a.stateF4, a.lists, a.count, a.ringOffF4, a.ringFrames, a.ringG, a.snapTab, a.split, a.pack, a.sectionWords, staging);
		return hipGetLastError();
	}

	hipError_t LaunchRecurrentSnapshot(float* state, int capacity, const int* slots, int count, int numElems, uint32_t* staging, bool import, hipStream_t stream)
	{
		if (count <= 0 || numElems <= 0) return hipSuccess;
		g_snapshotLaunches++;
		hipLaunchKernelGGL(RecurrentSnapshotKernel, dim3((unsigned)((count + 255) / 256), (unsigned)numElems), dim3(256), 0, stream, state, capacity, slots, count,
			numElems, staging, import ? 1 : 0);
		return hipGetLastError();
	}
}
