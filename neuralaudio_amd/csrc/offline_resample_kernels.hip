// offline_resample_kernels.hip -- the two resampling stages of NA_RenderOfflineAtRate (resample.h): the sums of the
// streaming stages (resample_kernels.hip) over ONE row of any length instead of many rows of at most 2048 samples.  No reference
// counterpart.
//
// Shape of the work (60 s at 44.1 -> 48 kHz): 2.9 M outputs of 49 / 53 multiply-adds each, 4 bytes read and 4 written per output --
// bandwidth- and latency-bound, nothing to reuse but the input window.  Grid (output tile, job), 256 threads: a workgroup stages the
// input span of its tile once in LDS (2048 outputs at 44.1 -> 48 kHz: 1930 / 2282 floats, under 9 KB, so the 32-wave limit and not LDS
// sets the 8 workgroups per CU; the taps re-read across a tile edge are 2.5 % of the window), zero outside the signal, cleaned like the
// streaming up stage.  A wave walks consecutive outputs (coalesced stores; neighbouring lanes read neighbouring LDS words).  The
// coefficients come phase-major through L2 as in the streaming kernels: a 640-phase table (over 120 KB) does not fit LDS beside the window.
// Every output is the shared FMA chain of resample_tap.h.  The 64-bit tick of a tile's first output is divided once per workgroup
// (uniform); inside the tile ticks are 32-bit offsets from it (< 640 + 2048 * 640).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "resample.h"
#include "resample_tap.h"

namespace na
{
	namespace
	{
		constexpr int kOfflineThreads = 256;

		template <bool CLEAN>
		__device__ __forceinline__ void OfflineStage(const OfflineResampleJob* __restrict__ jobs)
		{
			extern __shared__ float win[];
			const OfflineResampleJob j = jobs[blockIdx.y];
			const long long o0 = (long long)blockIdx.x * j.tile;
			if (o0 >= j.nOut) return; // (uniform: a shorter job of the same grid)
			const int count = (int)(j.nOut - o0 < (long long)j.tile ? j.nOut - o0 : (long long)j.tile);
			const long long tickA = j.tick0 + o0 * (long long)j.step;
			const long long idxA = tickA / j.period;
			const int r0 = (int)(tickA - idxA * j.period);
			const long long base = idxA - (j.taps - 1); // the input sample window index 0 holds
			for (int i = (int)threadIdx.x; i < j.window; i += kOfflineThreads)
			{
				const long long g = base + i;
				float v = 0.0f;
				if (g >= 0 && g < j.nIn)
				{
					v = j.in[g];
					if (CLEAN) v = ResampleCleanSample(v);
				}
				win[i] = v;
			}
			__syncthreads();
			float* __restrict__ out = j.out + o0;
			for (int o = (int)threadIdx.x; o < count; o += kOfflineThreads)
			{
				const int tick = r0 + o * j.step;
				const int q = tick / j.period;
				const int phase = tick - q * j.period;
				out[o] = ResampleTapSum(j.table + (long)phase * j.taps, win, q + j.taps - 1, j.taps, j.gain);
			}
		}
	}

	__global__ __launch_bounds__(kOfflineThreads) void OfflineResampleUpKernel(const OfflineResampleJob* __restrict__ jobs) { OfflineStage<true>(jobs); }
	__global__ __launch_bounds__(kOfflineThreads) void OfflineResampleDownKernel(const OfflineResampleJob* __restrict__ jobs) { OfflineStage<false>(jobs); }

	long long OfflineResampleWindow(int tile, int step, int period, int taps)
	{
		return (long long)taps + ((long long)(period - 1) + (long long)(tile - 1) * step) / period;
	}

	int OfflineResampleTile(int step, int period, int taps)
	{
		if (step < 1 || period < 1 || taps < 1) return 0;
		for (int tile = kOfflineResampleTile; tile >= 1; tile /= 2)
			if (OfflineResampleWindow(tile, step, period, taps) <= kOfflineResampleWindowFloats) return tile;
		return 0;
	}

	namespace
	{
		template <typename K>
		hipError_t LaunchOffline(K kernel, const OfflineResampleJob* jobs, const OfflineResampleJob* dJobs, int numJobs, hipStream_t stream)
		{
			if (numJobs <= 0) return hipSuccess;
			if (!jobs || !dJobs || numJobs > 65535) return hipErrorInvalidValue;
			long long tiles = 0;
			int window = 0;
			for (int i = 0; i < numJobs; i++)
			{
				const OfflineResampleJob& j = jobs[i];
				if (j.nIn < 0 || j.nOut < 0 || j.tick0 < 0 || j.step < 1 || j.period < 1 || j.taps < 1 || j.tile < 1 || j.tile > kOfflineResampleTile ||
					j.window < 1 || j.window > kOfflineResampleWindowFloats)
					return hipErrorInvalidValue;
				if (j.nOut == 0) continue;
				if (!j.in || !j.out || !j.table) return hipErrorInvalidValue;
				// ticks stay far inside 64 bits, a tile's own ticks inside 32
				if (j.nOut > (1LL << 40) || j.tick0 > (1LL << 60) || (long long)(j.period - 1) + (long long)(j.tile - 1) * j.step > 0x7fffffffLL) return hipErrorInvalidValue;
				// every window index an output of a tile forms lies inside the staged window, at any phase of the tile's first output:
				// the oldest is (taps - 1) - (taps - 1) = 0, the newest (taps - 1) + (period - 1 + (tile - 1) * step) / period
				const long long newest = (long long)(j.taps - 1) + ((long long)(j.period - 1) + (long long)(j.tile - 1) * j.step) / j.period;
				if (newest >= (long long)j.window) return hipErrorInvalidValue;
				tiles = std::max(tiles, (j.nOut + j.tile - 1) / j.tile);
				window = std::max(window, j.window);
			}
			if (tiles == 0) return hipSuccess;
			if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
			hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)numJobs), dim3(kOfflineThreads), (size_t)window * sizeof(float), stream, dJobs);
			return hipGetLastError();
		}
	}

	hipError_t LaunchOfflineResampleUp(const OfflineResampleJob* jobs, const OfflineResampleJob* dJobs, int numJobs, hipStream_t stream)
	{
		return LaunchOffline(OfflineResampleUpKernel, jobs, dJobs, numJobs, stream);
	}
	hipError_t LaunchOfflineResampleDown(const OfflineResampleJob* jobs, const OfflineResampleJob* dJobs, int numJobs, hipStream_t stream)
	{
		return LaunchOffline(OfflineResampleDownKernel, jobs, dJobs, numJobs, stream);
	}
}
