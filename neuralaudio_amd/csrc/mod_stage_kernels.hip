// mod_stage_kernels.hip -- the device side of the modulation stage (mod_stage.h): ONE launch per piece of a processing
// call with entries, over a table of the streams with a modulation only.  No reference counterpart (its hosts modulate on the CPU).
//
// The delay of a sample is fractional and moves, but it is a function of the sample's integer position alone (the LFO is an integer
// phase), so every read address of a piece is known up front: lanes run along the SAMPLES, the compressor's shape, not the delay's
// one-lane-per-stream walk.  A workgroup of four waves owns one entry and one LDS array, `line`:
//   line[0 .. reach)            the history the entry can reach, w[t0 - reach .. t0): coalesced loads from the row's ring, modulo
//                               ringSamples so a wrap can fall anywhere, +0 by POSITION where the line had not begun (hist)
//   line[reach .. reach + n)    the piece's own samples w[t0 .. t0 + n), computed in place behind the history
// so w[t - d] of sample j is line[reach + j - d], and every tap is an LDS gather at a computed index.  Afterwards the piece's part of
// the line goes back to the ring, coalesced.  The row is read and written sample by sample whatever its alignment: one path, so
// alignment and stride cannot show in the bits.
// Without feedback in either setting (chunk == 0) w = x': all lanes first file x' of the whole piece, one barrier, then every sample is
// independent.  With feedback the workgroup walks chunks of min(its width, floor(min base) - 1) samples -- no sample of a chunk reads
// what the chunk writes (mod_stage.h, the chunk rule) -- with one barrier between chunks; base = 2 is the serial extreme, chunks of 1.
// Static LDS: (4096 + 2048) floats = 24 KB.  The entry is read through a uniform address and stays in scalar registers.
#include <hip/hip_runtime.h>

#include <atomic>

#include "mod_stage.h"

namespace na
{
	namespace
	{
		constexpr int kModThreads = 256; // four waves, one entry
		std::atomic<unsigned long long> modLaunches{ 0 };

		// w[t - d] of the sample at `at`: `avail` floats lie in front of it (d never exceeds it for a table the book built: the bound only
		// keeps a read inside the array)
		struct ModLdsLine
		{
			const float* at;
			int avail;
			__device__ __forceinline__ float operator()(int d) const { return at[-min(max(d, 0), avail)]; }
		};
	}

	__global__ __launch_bounds__(kModThreads) void ModStageKernel(const ModLaunch L)
	{
		__shared__ float line[kModMaxDelaySamples + kModPieceSamples];
		const int tid = threadIdx.x;
		const ModEntry e = L.table[blockIdx.x];
		const int reach = min(max(e.reach, 0), kModMaxDelaySamples);
		const unsigned mask = (unsigned)L.ringSamples - 1u;
		float* const ring = L.rings + (long long)e.row * L.ringSamples;
		float* const row = L.rows + (long long)e.row * L.stride + (long long)L.done;
		const long long held = (long long)e.hist + (long long)L.done; // samples of the line in front of the piece
		const unsigned p0 = e.pos + (unsigned)L.done;                // where the piece's first sample goes (ringSamples divides 2^32)
		const long long k0 = (long long)e.k + (long long)L.done;     // the fade's position at the piece's first sample
		// a fade to none retires with the sample at which it ends: the rest of the row is not touched
		const int live = e.toNone ? (int)max(0ll, min((long long)L.n, (long long)e.N - k0)) : L.n;
		for (int i = tid; i < reach; i += kModThreads)
		{
			const int back = reach - i;
			line[i] = (long long)back <= held ? ring[(p0 - (unsigned)back) & mask] : 0.0f;
		}
		float* const now = line + reach;
		if (e.chunk == 0)
		{
			for (int j = tid; j < live; j += kModThreads) now[j] = ModInput(row[j]);
			__syncthreads();
			for (int j = tid; j < live; j += kModThreads)
			{
				float w;
				// (x' of x' is x')
				row[j] = ModStep(e, k0 + j, L.done + (unsigned long long)j, now[j], ModLdsLine{ now + j, reach + j }, w);
			}
		}
		else
		{
			__syncthreads();
			const int chunk = min(kModThreads, e.chunk);
			for (int c0 = 0; c0 < live; c0 += chunk)
			{
				const int j = c0 + tid;
				if (tid < chunk && j < live)
				{
					float w;
					row[j] = ModStep(e, k0 + j, L.done + (unsigned long long)j, row[j], ModLdsLine{ now + j, reach + j }, w);
					now[j] = w;
				}
				__syncthreads();
			}
		}
		__syncthreads();
		for (int j = tid; j < live; j += kModThreads) ring[(p0 + (unsigned)j) & mask] = now[j];
	}

	hipError_t LaunchModStage(const ModLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n <= 0) return hipSuccess;
		if (!L.table || !L.rows || !L.rings || L.n > kModPieceSamples || L.ringSamples < kModMinDelaySamples + kModPieceSamples || (L.ringSamples & (L.ringSamples - 1)) != 0)
			return hipErrorInvalidValue;
		hipLaunchKernelGGL(ModStageKernel, dim3((unsigned)L.count), dim3(kModThreads), 0, stream, L);
		modLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long ModStageLaunches() { return modLaunches.load(std::memory_order_relaxed); }
}
