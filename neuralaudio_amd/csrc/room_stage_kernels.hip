// room_stage_kernels.hip -- the device side of the room stage (room_stage.h): ONE launch per processing call with
// entries, over a table of the streams with a room only.  No reference counterpart (its hosts run their reverb on the CPU).
//
// A feedback delay network looks serial, but every line is at least kRoomPieceSamples = 128 samples long and the damping is a two-tap
// FIR, not a recursion: the 128 samples of a piece read nothing the piece writes.  So lanes run along the SAMPLES, the modulation
// stage's shape, not the delay stage's one-lane-per-stream walk.  A workgroup of two waves owns one entry; thread j owns sample j of
// the piece and holds all eight lines of it in registers, so the Hadamard mix is 24 adds inside the thread: no cross-lane traffic and
// no barrier inside a sample.
//   win[1][i][0 .. 128]   the window of line i a piece reads, L_i[t0 - len_i - 1 .. t0 - len_i + 127]: coalesced loads from the row's
//                         ring i, modulo ringSamples so a wrap can fall anywhere, +0 by POSITION where the line had not begun (hist).
//                         Sample j reads q_i at [j] and r_i at [j + 1]: neighbouring samples share a tap, neighbouring lanes
//                         neighbouring banks.
//   win[0][i][..]         the same window at the length the line fades FROM, only while a set call that changed len_i is fading
// The row's sample goes straight to its thread (neighbouring lanes, neighbouring words: coalesced whatever the alignment -- one path, so
// alignment and stride cannot show in the bits); the eight new line samples and y go back the same way, in place.
// A call longer than a piece is a loop over pieces inside the one launch, on the same workgroup: a later piece reads what an earlier
// one stored (at len_i = 128 the very last sample of it), so a workgroup-scope fence on global memory and a barrier stand between the
// stores of a piece and the loads of the next.
// The two settings of the entry's fade live in a block per row on the device; a set call's settings come behind the entries of the
// next table, once, and the launch files them.  Entry and setting are read through uniform addresses before anything is stored.
// Static LDS: 2 x 8 x 129 floats = 8.1 KB an entry.
// NA_ROOM_GROUP_ENTRIES (a build knob of this file alone, profiles/room_cost.txt): 2 lets a workgroup of four waves serve two entries.
#include <hip/hip_runtime.h>

#include <atomic>

#include "room_stage.h"

#ifndef NA_ROOM_GROUP_ENTRIES
#define NA_ROOM_GROUP_ENTRIES 1
#endif

namespace na
{
	namespace
	{
		constexpr int kRoomGroupEntries = NA_ROOM_GROUP_ENTRIES;                // entries of one workgroup
		constexpr int kRoomThreads = kRoomPieceSamples * kRoomGroupEntries;     // two waves an entry
		constexpr int kRoomSetWords = (int)(sizeof(RoomSetting) / sizeof(int));
		static_assert(kRoomGroupEntries == 1 || kRoomGroupEntries == 2, "one or two entries a workgroup");
		static_assert(kRoomSetWords <= kRoomPieceSamples, "an entry's threads file its setting in one pass");
		std::atomic<unsigned long long> roomLaunches{ 0 };

		// L_i[t - len - back] of sample j: the windows begin at t0 - len - 1
		struct RoomLdsTap
		{
			const float (*win)[kRoomLines][kRoomWindow];
			int j;
			__device__ __forceinline__ float operator()(int i, bool a, int back) const { return win[a ? 0 : 1][i][j + 1 - back]; }
		};
	}

	__global__ __launch_bounds__(kRoomThreads) void RoomStageKernel(const RoomLaunch L)
	{
		__shared__ float win[kRoomGroupEntries][2][kRoomLines][kRoomWindow];
		// (the waves of an entry agree on it: the entry and its setting stay in scalar registers)
		const int sub = kRoomGroupEntries == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x / kRoomPieceSamples);
		const int j = (int)threadIdx.x % kRoomPieceSamples;
		const int index = (int)blockIdx.x * kRoomGroupEntries + sub;
		const bool mine = index < L.count; // (an odd count leaves the last workgroup's second half idle: it only keeps the barriers)
		const RoomEntry e = L.table[mine ? index : 0];
		const RoomSetting* const from = e.set >= 0 ? reinterpret_cast<const RoomSetting*>(L.table + L.count) + e.set : L.settings + e.row;
		const RoomSetting g = *from;
		if (mine && e.set >= 0 && j < kRoomSetWords) reinterpret_cast<int*>(L.settings + e.row)[j] = reinterpret_cast<const int*>(from)[j];

		const unsigned mask = (unsigned)L.ringSamples - 1u;
		float* const rings = L.rings + (long long)e.row * kRoomLines * L.ringSamples;
		float* const row = L.rows + (long long)e.row * L.stride;
		for (unsigned long long done = 0; done < L.n; done += (unsigned long long)kRoomPieceSamples)
		{
			const int len = (int)min((unsigned long long)kRoomPieceSamples, L.n - done);
			const long long held = (long long)e.hist + (long long)done; // samples of the lines in front of the piece
			const unsigned p0 = e.pos + (unsigned)done;                 // where the piece's first sample goes (ringSamples divides 2^32)
			const long long k0 = (long long)e.k + (long long)done;      // the fade's position at the piece's first sample
			// a fade to none retires with the sample at which it ends: the rest of the row is not touched
			const int live = !mine ? 0 : e.toNone ? (int)max(0ll, min((long long)len, (long long)e.N - k0)) : len;
			const bool fading = k0 < (long long)e.N - 1;                // the piece's first sample has wk < 1
			if (live > 0)
			{
#pragma unroll
				for (int i = 0; i < kRoomLines; i++)
				{
					const float* const ring = rings + (long long)i * L.ringSamples;
					const bool blend = fading && g.lenA[i] != g.lenB[i];
					for (int w = j; w < kRoomWindow; w += kRoomPieceSamples)
					{
						const int backB = g.lenB[i] + 1 - w; // >= 1: a line is at least a piece long
						win[sub][1][i][w] = (long long)backB <= held ? ring[(p0 - (unsigned)backB) & mask] : 0.0f;
						if (blend)
						{
							const int backA = g.lenA[i] + 1 - w;
							win[sub][0][i][w] = (long long)backA <= held ? ring[(p0 - (unsigned)backA) & mask] : 0.0f;
						}
					}
				}
			}
			__syncthreads();
			if (j < live)
			{
				float line[kRoomLines];
				const float wk = OutStageWeightAt(e.N, k0 + j);
				row[done + j] = RoomStep(g, wk, row[done + j], RoomLdsTap{ win[sub], j }, line);
#pragma unroll
				for (int i = 0; i < kRoomLines; i++) rings[(long long)i * L.ringSamples + ((p0 + (unsigned)j) & mask)] = line[i];
			}
			// the next piece's windows read what this one stored
			__threadfence_block();
			__syncthreads();
		}
	}

	hipError_t LaunchRoomStage(const RoomLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rows || !L.rings || !L.settings || L.ringSamples < kRoomMinMaxLine + kRoomWindow || (L.ringSamples & (L.ringSamples - 1)) != 0)
			return hipErrorInvalidValue;
		hipLaunchKernelGGL(RoomStageKernel, dim3((unsigned)((L.count + kRoomGroupEntries - 1) / kRoomGroupEntries)), dim3(kRoomThreads), 0, stream, L);
		roomLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long RoomStageLaunches() { return roomLaunches.load(std::memory_order_relaxed); }
}
