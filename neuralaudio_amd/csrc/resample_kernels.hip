// resample_kernels.hip -- the two stages of a resampling batch (resample.h): ResampleUpKernel (external rate -> model
// rate, in front of the model launches) and ResampleDownKernel (model rate -> external rate, behind them).  No reference counterpart.
//
// Shape of the work (1024 streams x 128 external frames at 44.1 -> 48 kHz): 139 x 49 + 128 x 53 multiply-adds and ~2.6 KB per stream
// and call -- launch- and latency-bound.  One launch per stage for the whole batch, one workgroup per row: the row's window (its history
// ++ this call's samples) is staged once in LDS, a wave walks consecutive outputs of the row (coalesced stores; neighbouring lanes read
// neighbouring LDS words, two lanes on one word are a broadcast), every output is ONE sum over its taps in a fixed order -- no atomics,
// no split sums -- so the result does not depend on how the signal was cut into calls.  The coefficients are read phase-major through
// L2 (a phase's taps are consecutive: 49 x 4 bytes per output, the whole 44.1 -> 48 kHz table is 31 KB and stays cached).  The same
// workgroup hands the history over: it writes the row's new history from LDS after the barrier behind every read of the old one.
#include <hip/hip_runtime.h>

#include "resample.h"
#include "resample_tap.h"

namespace na
{
	namespace
	{
		constexpr int kResampleThreads = 256;

		template <bool CLEAN>
		__device__ __forceinline__ void ResampleStage(const ResampleStageArgs& a)
		{
			extern __shared__ float win[];
			const int row = (int)blockIdx.x;
			const float* __restrict__ in = a.in + (long)row * a.inStride;
			float* __restrict__ hist = a.hist + (long)row * a.histLen;
			const int window = a.histLen + a.nIn;
			for (int i = (int)threadIdx.x; i < window; i += kResampleThreads)
			{
				float v;
				if (i < a.histLen) v = hist[i];
				else
				{
					v = in[i - a.histLen];
					if (CLEAN) v = ResampleCleanSample(v);
				}
				win[i] = v;
			}
			__syncthreads();
			float* __restrict__ out = a.out + (long)row * a.outStride;
			for (int o = (int)threadIdx.x; o < a.nOut; o += kResampleThreads)
			{
				const int tick = a.tick0 + o * a.step;
				const int idx = tick / a.period;
				const int phase = tick - idx * a.period;
				// (the sum itself is shared with the offline stages: resample_tap.h)
				out[o] = ResampleTapSum(a.table + (long)phase * a.taps, win, idx, a.taps, a.gain);
			}
			// (every read of the old history happened in front of the barrier)
			for (int i = (int)threadIdx.x; i < a.histLen; i += kResampleThreads) hist[i] = win[a.nIn + i];
		}
	}

	__global__ __launch_bounds__(kResampleThreads) void ResampleUpKernel(const ResampleStageArgs a) { ResampleStage<true>(a); }
	__global__ __launch_bounds__(kResampleThreads) void ResampleDownKernel(const ResampleStageArgs a) { ResampleStage<false>(a); }

	namespace
	{
		template <typename K>
		hipError_t LaunchStage(K kernel, const ResampleStageArgs& a, hipStream_t stream)
		{
			if (a.rows <= 0) return hipSuccess;
			const size_t window = (size_t)a.histLen + (size_t)a.nIn;
			if (window > (size_t)kResampleWindowFloats || a.nIn < 0 || a.nOut < 0 || a.taps < 1 || a.period < 1 || a.step < 1 || a.tick0 < 0) return hipErrorInvalidValue;
			// every window index an output reads lies inside the window (the host's arithmetic, checked where it would become an address)
			if (a.nOut > 0)
			{
				const long long first = (long long)a.tick0 / a.period - (a.taps - 1);
				const long long last = ((long long)a.tick0 + (long long)(a.nOut - 1) * a.step) / a.period;
				if (first < 0 || last >= (long long)window) return hipErrorInvalidValue;
			}
			hipLaunchKernelGGL(kernel, dim3((unsigned)a.rows), dim3(kResampleThreads), window * sizeof(float), stream, a);
			return hipGetLastError();
		}
	}

	hipError_t LaunchResampleUp(const ResampleStageArgs& a, hipStream_t stream) { return LaunchStage(ResampleUpKernel, a, stream); }
	hipError_t LaunchResampleDown(const ResampleStageArgs& a, hipStream_t stream) { return LaunchStage(ResampleDownKernel, a, stream); }
}
