// tuner_stage_kernels.hip -- the device side of the tuner stage (tuner_stage.h): per piece of a processing call with
// entries ONE append launch over a table of the streams with a tuner and, only where an evaluation ends in the piece, ONE evaluate
// launch over those of them that evaluate.  Both run in front of the model launches (the input rows may be the output rows) and neither
// writes an audio row.  No reference counterpart (its hosts tune on the CPU).
//
// TunerAppendKernel: one wave per entry, lanes along the decimated samples -- lane l takes groups l, l + 64, ... of the piece, D
// neighbouring floats each (TunerGroupSum: quantise, sum) -- and stores them as int32 into the row's ring at their own index, so the
// ring's contents do not depend on the cut.  Groups are aligned to the tuner's position 0: lane 0 joins the carried part of the
// group that was open when the piece began (TunerState::partial) to its first group and leaves the part of the group that stays
// open; a piece shorter than D only adds to it.
//
// TunerEvaluateKernel: one workgroup of four waves per evaluating entry.  The W + maxLag + 2 ring values behind the evaluation's end go
// to LDS (indices below 0 read as 0: nothing from before the tuner's position 0 is ever read, so no memset travels with a set
// call); lanes run along the lags -- thread l owns lags l, l + 256, ... -- so d[m - j] is one address for the wave and d[m - j - t]
// consecutive ones; the sums are 64-bit integers (TunerLagSums: a thread's lags side by side, so that the chains of multiply-adds of
// a wave that is alone on its SIMD overlap) and land in LDS, where the selection -- a min of t, a 64-bit max, a min of t -- is three
// LDS integer reductions across the workgroup.  e[] is summed for the three lags a reading holds only (the selection does not look at
// it).  No float instruction runs behind TunerQuantise.
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>

#include "tuner_stage.h"

namespace na
{
	namespace
	{
		constexpr int kTunerAppendLanes = 64;   // one wave per entry
		constexpr int kTunerEvalThreads = 256;  // four waves per evaluation
		constexpr int kTunerRingMask = kTunerRingSamples - 1;
		std::atomic<unsigned long long> tunerLaunches{ 0 };

		static_assert((kTunerMaxLag + 2 + kTunerEvalThreads - 1) / kTunerEvalThreads <= 5, "a thread owns five lags at the most");
		// r[tid], r[tid + 256], ... of the N lags the thread owns; a lag past `top` is summed as lag 0 (in bounds) and dropped
		template <int N>
		__device__ __forceinline__ void ThreadLags(const int* span, int span_n, int W, int top, int tid, long long* r)
		{
			int t[N];
			long long sum[N];
			for (int i = 0; i < N; i++)
			{
				const int lag = tid + i * kTunerEvalThreads;
				t[i] = lag <= top ? lag : 0;
			}
			TunerLagSums<N>(span, span_n, W, t, sum);
			for (int i = 0; i < N; i++)
			{
				const int lag = tid + i * kTunerEvalThreads;
				if (lag <= top) r[lag] = sum[i];
			}
		}
	}

	__global__ __launch_bounds__(kTunerAppendLanes) void TunerAppendKernel(const TunerLaunch L)
	{
		const int lane = threadIdx.x;
		const TunerEntry e = L.table[blockIdx.x];
		if (e.row < 0 || e.decimation < 1 || e.decimation > kTunerMaxDecimation) return;
		const int D = e.decimation;
		TunerState* st = L.state + e.row;
		const float* __restrict__ x = L.rows + (long long)e.row * L.stride + (long long)L.offset;
		int* __restrict__ ring = L.rings + (long long)e.row * kTunerRingSamples;
		const unsigned long long first = e.pos + L.offset, end = first + L.n; // positions [first, end)
		const long long mFirst = (long long)(first / (unsigned long long)D);  // the group that holds `first`
		const long long mEnd = (long long)(end / (unsigned long long)D);      // groups [mFirst, mEnd) are complete behind this piece
		// (position 0 of a tuner is the start of a group: a start code never meets a carried part)
		const bool carried = first % (unsigned long long)D != 0 && !(e.start == kTunerStartFresh && L.offset == 0);
		const int old = (lane == 0 && carried) ? st->partial : 0;
		for (long long m = mFirst + lane; m < mEnd; m += kTunerAppendLanes)
		{
			int d = TunerGroupSum(x, first, L.n, m, D);
			if (m == mFirst) d += old;
			ring[m & kTunerRingMask] = d;
		}
		if (lane != 0) return;
		TunerState next;
		next.partial = (mEnd == mFirst ? old : 0) + TunerGroupSum(x, first, L.n, mEnd, D); // the group that stays open
		next.gen = e.gen;
		*st = next;
	}

	__global__ __launch_bounds__(kTunerEvalThreads) void TunerEvaluateKernel(const TunerLaunch L)
	{
		__shared__ int span[kTunerMaxSpan];
		__shared__ long long r[kTunerMaxLag + 2];
		__shared__ unsigned long long rMax, eSum[3];
		__shared__ int zMin, lagMin;
		const int tid = threadIdx.x;
		const int index = L.table[blockIdx.x].evalEntry;
		if (index < 0 || index >= L.count) return;
		const TunerEntry e = L.table[index];
		if (e.row < 0 || e.evalM < 0 || e.decimation < 1) return;
		if (e.window < kTunerMinWindow || e.window > kTunerMaxWindow || e.maxLag < kTunerMinMaxLag || e.maxLag > kTunerMaxLag) return;
		// the piece that holds the evaluation's last sample runs it: everything it reads is in the ring, nothing behind it has been overwritten
		const unsigned long long last = (unsigned long long)(e.evalM + 1) * (unsigned long long)e.decimation - 1ull;
		if (last < e.pos + L.offset || last >= e.pos + L.offset + L.n) return;
		const int W = e.window, top = e.maxLag + 1, span_n = W + e.maxLag + 2;
		const int* __restrict__ ring = L.rings + (long long)e.row * kTunerRingSamples;
		for (int i = tid; i < span_n; i += kTunerEvalThreads)
		{
			const long long m = e.evalM - (long long)(span_n - 1) + i;
			span[i] = m < 0 ? 0 : ring[m & kTunerRingMask];
		}
		if (tid == 0)
		{
			zMin = INT_MAX;
			lagMin = INT_MAX;
			rMax = 0ull;
			eSum[0] = eSum[1] = eSum[2] = 0ull;
		}
		__syncthreads();
		// (a thread's lags are summed side by side: one d[m - j] read for all of them and independent chains of multiply-adds)
		switch ((top + kTunerEvalThreads) / kTunerEvalThreads)
		{
		case 1: ThreadLags<1>(span, span_n, W, top, tid, r); break;
		case 2: ThreadLags<2>(span, span_n, W, top, tid, r); break;
		case 3: ThreadLags<3>(span, span_n, W, top, tid, r); break;
		case 4: ThreadLags<4>(span, span_n, W, top, tid, r); break;
		default: ThreadLags<5>(span, span_n, W, top, tid, r); break;
		}
		__syncthreads();
		const bool loud = (unsigned long long)r[0] >= e.minEnergy;
		for (int t = tid; t <= top; t += kTunerEvalThreads)
			if (t >= 1 && r[t] <= 0) atomicMin(&zMin, t);
		__syncthreads();
		const int z = zMin;
		const bool search = loud && z != INT_MAX;
		if (search)
			for (int t = tid; t <= e.maxLag; t += kTunerEvalThreads)
				if (t >= 1 && TunerIsCandidate(r[t - 1], r[t], r[t + 1], t, z, e.minLag, e.maxLag)) atomicMax(&rMax, (unsigned long long)r[t]);
		__syncthreads();
		const long long rmax = (long long)rMax;
		if (search && rmax > 0)
			for (int t = tid; t <= e.maxLag; t += kTunerEvalThreads)
				if (t >= 1 && TunerIsCandidate(r[t - 1], r[t], r[t + 1], t, z, e.minLag, e.maxLag) && TunerPasses(r[t], e.thresholdQ10, rmax)) atomicMin(&lagMin, t);
		__syncthreads();
		const int lag = lagMin == INT_MAX ? 0 : lagMin;
		if (lag > 0)
		{
			// e[lag - 1], e[lag], e[lag + 1]: threads along j
			unsigned long long sum[3] = { 0ull, 0ull, 0ull };
			for (int j = tid; j < W; j += kTunerEvalThreads)
				for (int i = 0; i < 3; i++)
				{
					const long long v = span[span_n - 1 - j - (lag - 1 + i)];
					sum[i] += (unsigned long long)(v * v);
				}
			for (int i = 0; i < 3; i++) atomicAdd(&eSum[i], sum[i]);
		}
		__syncthreads();
		if (tid != 0) return;
		TunerRecord rec;
		rec.row = e.row;
		rec.gen = e.gen;
		rec.reading.evaluations = e.evaluations;
		rec.reading.position = (e.evalM + 1) * (long long)e.decimation;
		rec.reading.e0 = (unsigned long long)r[0];
		for (int i = 0; i < 3; i++)
		{
			rec.reading.r[i] = lag > 0 ? r[lag - 1 + i] : 0;
			rec.reading.e[i] = lag > 0 ? eSum[i] : 0ull;
		}
		rec.reading.lag = lag;
		rec.reading.decimation = e.decimation;
		L.results[blockIdx.x] = rec;
	}

	hipError_t LaunchTunerAppend(const TunerLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rows || !L.state || !L.rings || L.n > (unsigned long long)kTunerPieceSamples) return hipErrorInvalidValue;
		hipLaunchKernelGGL(TunerAppendKernel, dim3((unsigned)L.count), dim3(kTunerAppendLanes), 0, stream, L);
		tunerLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	hipError_t LaunchTunerEvaluate(const TunerLaunch& L, hipStream_t stream)
	{
		if (L.evaluating <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rings || !L.results || L.evaluating > L.count || L.n > (unsigned long long)kTunerPieceSamples) return hipErrorInvalidValue;
		hipLaunchKernelGGL(TunerEvaluateKernel, dim3((unsigned)L.evaluating), dim3(kTunerEvalThreads), 0, stream, L);
		tunerLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long TunerStageLaunches() { return tunerLaunches.load(std::memory_order_relaxed); }
}
