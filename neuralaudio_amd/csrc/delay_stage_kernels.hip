// delay_stage_kernels.hip -- the device side of the delay stage (delay_stage.h): ONE launch per piece of a processing
// call with entries, over a table of the streams with a delay only.  No reference counterpart (its hosts delay on the CPU).
//
// The recurrence is strictly serial per stream -- sample t needs sample t - D of the stage's own line, through two one-pole filters --
// so the only parallelism is across entries: the gate detector's shape.  One lane per entry, 64 entries to a workgroup of one wave.
// Tiles of 64 entries x 64 samples move through LDS row by row (neighbouring lanes on neighbouring samples: coalesced global accesses,
// one path for every alignment and stride), each lane then walks ITS row of the tiles.  The tiles' row stride is 65 floats: lane e
// reads word e * 65 + j, so the 64 lanes fall on 64 different banks.
//
// Three tiles: the row's samples x (the outputs y replace them and leave the way they came); the line, which arrives holding the
// delayed samples w[t - D_B] of the tile -- fetched from the entry's own ring offset, sample by sample modulo ringSamples, so a wrap can
// fall anywhere -- and leaves holding the new samples w[t] of the tile, back to the ring the coalesced way; and, only for an entry whose
// read head cross-fades, the delayed samples w[t - D_A].  The line tile is overwritten in place: at step j the lane first reads what it
// needs, then stores w at j.  Where D is shorter than the tile the sample t - D was produced earlier in the SAME tile and the staged
// copy at j is stale: the lane reads index j - D of the line tile, which holds what it wrote, for every j >= D (and nothing is fetched
// for those).  A read in front of T0 yields +0 by comparing positions (hist), never by what the ring holds.
// l, q and the position stay in registers across the tiles of a piece; the state is stored once per piece.
// 3 x 64 x 65 floats = 49.9 KB of LDS.  What a launch costs is one wave's dependent chain over n samples.
#include <hip/hip_runtime.h>

#include <atomic>

#include "delay_stage.h"

namespace na
{
	namespace
	{
		constexpr int kDelayLanes = 64;       // entries of one workgroup (one wave)
		constexpr int kDelayTileSamples = 64; // samples of a tile
		constexpr int kDelayTileStride = kDelayTileSamples + 1; // (odd: the lanes' rows start on different banks)
		std::atomic<unsigned long long> delayLaunches{ 0 };
	}

	__global__ __launch_bounds__(kDelayLanes) void DelayStageKernel(const DelayLaunch L)
	{
		__shared__ float xt[kDelayLanes * kDelayTileStride]; // x in, y out
		__shared__ float wt[kDelayLanes * kDelayTileStride]; // w[t - D_B] in, w[t] out
		__shared__ float at[kDelayLanes * kDelayTileStride]; // w[t - D_A] in (head cross-fade only)
		__shared__ int rowOf[kDelayLanes], headA[kDelayLanes], headB[kDelayLanes], histOf[kDelayLanes];
		__shared__ unsigned posOf[kDelayLanes];
		const int lane = threadIdx.x;
		const int first = blockIdx.x * kDelayLanes;
		const int here = min(kDelayLanes, L.count - first); // entries of this workgroup
		const bool mine = lane < here;
		const unsigned mask = (unsigned)L.ringSamples - 1u;
		DelayEntry e;
		DelayFilter s;
		if (mine)
		{
			e = L.table[first + lane];
			if (e.start && L.done == 0) s = DelayFilter();
			else s = L.state[e.row];
		}
		const bool blend = mine && e.N > 0 && e.DA != e.DB; // (the fade's end inside the call only makes the A head unused)
		rowOf[lane] = mine ? e.row : -1;
		headA[lane] = blend ? e.DA : 0; // 0: no A head
		headB[lane] = mine ? e.DB : 1;
		histOf[lane] = mine ? e.hist : 0;
		posOf[lane] = mine ? e.pos : 0u;
		__syncthreads();
		for (int t0 = 0; t0 < L.n; t0 += kDelayTileSamples)
		{
			const int len = min(kDelayTileSamples, L.n - t0);
			const unsigned long long i0 = L.done + (unsigned long long)t0; // the tile's first sample, counted in the call
			// in: row r of the tiles is entry r's, lanes along the samples
			if (lane < len)
			{
				for (int r = 0; r < here; r++)
				{
					const float* src = L.rows + (long long)rowOf[r] * L.stride + (long long)i0;
					const float* ring = L.rings + (long long)rowOf[r] * L.ringSamples;
					const long long held = (long long)histOf[r] + (long long)i0 + lane; // samples of the line in front of this one
					const unsigned p = posOf[r] + (unsigned)i0 + (unsigned)lane;        // (ringSamples divides 2^32)
					const int DB = headB[r], DA = headA[r];
					xt[r * kDelayTileStride + lane] = src[lane];
					if (lane < DB) wt[r * kDelayTileStride + lane] = held >= DB ? ring[(p - (unsigned)DB) & mask] : 0.0f;
					if (lane < DA) at[r * kDelayTileStride + lane] = held >= DA ? ring[(p - (unsigned)DA) & mask] : 0.0f;
				}
			}
			__syncthreads();
			if (mine)
			{
				float* mx = xt + lane * kDelayTileStride;
				float* mw = wt + lane * kDelayTileStride;
				const float* ma = at + lane * kDelayTileStride;
				const long long k0 = (long long)e.k + (long long)i0;
				for (int j = 0; j < len; j++)
				{
					const long long k = k0 + j;
					if (e.toNone && k >= e.N) break; // retired with the sample at which the fade ended: the rest of the row is not touched
					const float wk = OutStageWeightAt(e.N, k);
					const float dB = j >= e.DB ? mw[j - e.DB] : mw[j];
					float dA = 0.0f;
					if (blend && wk != 1.0f) dA = j >= e.DA ? mw[j - e.DA] : ma[j];
					float w;
					mx[j] = DelayStep(e, s, wk, mx[j], dA, dB, w);
					mw[j] = w;
				}
			}
			__syncthreads();
			// out: the outputs the way the samples came, the line to the ring
			if (lane < len)
			{
				for (int r = 0; r < here; r++)
				{
					float* dst = L.rows + (long long)rowOf[r] * L.stride + (long long)i0;
					float* ring = L.rings + (long long)rowOf[r] * L.ringSamples;
					const unsigned p = posOf[r] + (unsigned)i0 + (unsigned)lane;
					dst[lane] = xt[r * kDelayTileStride + lane];
					ring[p & mask] = wt[r * kDelayTileStride + lane];
				}
			}
			__syncthreads(); // (also: the ring's new samples are visible to the next tile's fetches of this workgroup)
		}
		if (mine) L.state[e.row] = s;
	}

	hipError_t LaunchDelayStage(const DelayLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n <= 0) return hipSuccess;
		if (!L.table || !L.rows || !L.rings || !L.state || L.n > kDelayPieceSamples || L.ringSamples < kDelayPieceSamples || (L.ringSamples & (L.ringSamples - 1)) != 0)
			return hipErrorInvalidValue;
		hipLaunchKernelGGL(DelayStageKernel, dim3((unsigned)((L.count + kDelayLanes - 1) / kDelayLanes)), dim3(kDelayLanes), 0, stream, L);
		delayLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long DelayStageLaunches() { return delayLaunches.load(std::memory_order_relaxed); }
}
