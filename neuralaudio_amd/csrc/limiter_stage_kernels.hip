// limiter_stage_kernels.hip -- the device side of the limiter stage (limiter_stage.h): ONE launch per piece of a
// processing call with entries, over a table of the streams with a limiter only.  No reference counterpart (its hosts limit on the CPU).
//
// The limiter is feed-forward: a sliding minimum and a fixed-order sum, nothing recurs in time, so lanes run along the SAMPLES.  A
// workgroup of four waves owns one entry (a row) and one piece.  The row is processed in place and a sample reads K = 2 L + H input
// samples behind it, so the workgroup first brings everything it reads into LDS -- the K samples in front of the piece from the row's
// history ring (+0 by POSITION where the entry had not begun), then the piece itself from the row --, barriers, and only then stores:
//   a, b  [K + n]   need of every sample, then the doubling passes ping-pong between the two:
//                   M_(j+1)[i] = min(M_j[i - 2^j], M_j[i]) up to the largest 2^p <= W = L + H + 1; m[i] = min(M_p[i - (W - 2^p)], M_p[i])
//                   (two overlapping powers of two cover the window; a minimum is exact, so its order is free); then the contract's
//                   pairwise tree S_(j+1)[i] = S_j[i - 2^j] + S_j[i], log2 L passes, in exactly the stated order
//   xs    [L + n]   the samples themselves from L in front of the piece on: x[t - L] of the outputs, and what goes back to the ring
// Index i of a and b is the sample K - i in front of the piece's first (i >= K: sample i - K of the piece).  m is valid from
// K - L + 1 on and S_j from K - L + 2^j on: S of every sample of the piece is the full tree; what lies in front is scratch.
// LDS is dynamic, sized by the largest K and L among the launch's entries: (2 (K + n) + n + L) floats, 54 KB at the maxima with a
// piece of 1024, a few KB for a 128-sample buffer with a short window.  No atomics, no inline assembly, no transcendental.
#include <hip/hip_runtime.h>

#include <atomic>

#include "limiter_stage.h"

namespace na
{
	namespace
	{
		constexpr int kLimThreads = 256; // four waves, one entry
		std::atomic<unsigned long long> limLaunches{ 0 };
	}

	__global__ __launch_bounds__(kLimThreads) void LimiterStageKernel(const LimiterLaunch Lc)
	{
		extern __shared__ float limLds[];
		const int tid = threadIdx.x;
		const LimiterEntry e = Lc.table[blockIdx.x];
		const int L = e.lookahead, n = Lc.n;
		const int K = 2 * L + e.hold, W = L + e.hold + 1;
		// (a table the book built passes; the test only keeps every index below inside the launch's arrays)
		if (e.row < 0 || e.row >= Lc.rowCapacity || L < kLimMinLookahead || L > Lc.maxLookahead || e.hold < 0 || K > Lc.maxWindow || (1 << e.logL) != L) return;
		const int span = Lc.maxWindow + n, total = K + n;
		float* src = limLds;
		float* dst = limLds + span;
		float* const xs = limLds + 2 * span;
		float* const ring = Lc.history + (long long)e.row * kLimHistory;
		float* const row = Lc.rows + (long long)e.row * Lc.stride + (long long)Lc.done;
		const long long held = (long long)e.held + (long long)Lc.done;                                 // the entry's samples in front of the piece
		const int p0 = (int)(((unsigned long long)e.ringPos + Lc.done) % (unsigned long long)kLimHistory); // where the piece's first sample goes
		const long long k0 = e.done + (long long)Lc.done;                                              // the ramp's position at the piece's first sample

		// everything the piece reads, before anything is written: need of every sample, the samples from L in front of the piece on
		for (int i = tid; i < total; i += kLimThreads)
		{
			float v;
			if (i < K)
			{
				const int back = K - i;
				int at = p0 - back;
				if (at < 0) at += kLimHistory;
				v = (long long)back <= held ? ring[at] : 0.0f;
			}
			else v = row[i - K];
			src[i] = LimNeed(v, LimCeilingAt(e.from, e.to, e.R, k0 + (long long)(i - K)));
			if (i >= K - L) xs[i - (K - L)] = v;
		}
		__syncthreads();

		// the sliding minimum over W samples: doubling passes up to the largest power of two in W, then two of them side by side
		int s = 1;
		for (; 2 * s <= W; s *= 2)
		{
			for (int i = tid; i < total; i += kLimThreads) dst[i] = i >= s ? fminf(src[i - s], src[i]) : src[i];
			__syncthreads();
			float* const t = src;
			src = dst;
			dst = t;
		}
		const int first = K - L + 1, off = W - s; // m is read from `first` on; first - off = s >= 0
		for (int i = first + tid; i < total; i += kLimThreads) dst[i] = fminf(src[i - off], src[i]);
		__syncthreads();
		{
			float* const t = src;
			src = dst;
			dst = t;
		}

		// the pairwise tree over the last L values of m, in the contract's order
		for (s = 1; s < L; s *= 2)
		{
			for (int i = first + tid; i < total; i += kLimThreads)
			{
				const float newer = src[i];
				dst[i] = i - s >= first ? src[i - s] + newer : newer;
			}
			__syncthreads();
			float* const t = src;
			src = dst;
			dst = t;
		}

		// the delayed sample times the gain, clamped; the piece's own samples go to the ring
		const float invL = 1.0f / (float)L;
		for (int j = tid; j < n; j += kLimThreads)
		{
			row[j] = LimOutput(xs[j], src[K + j], invL, LimCeilingAt(e.from, e.to, e.R, k0 + (long long)j));
			int at = p0 + j;
			if (at >= kLimHistory) at -= kLimHistory;
			ring[at] = xs[L + j];
		}
	}

	hipError_t LaunchLimiterStage(const LimiterLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n <= 0) return hipSuccess;
		if (!L.table || !L.rows || !L.history || L.n > kLimPieceSamples || L.rowCapacity <= 0 || L.maxWindow < 2 * kLimMinLookahead || L.maxWindow > kLimHistory ||
			L.maxLookahead < kLimMinLookahead || L.maxLookahead > kLimMaxLookahead)
			return hipErrorInvalidValue;
		const size_t lds = ((size_t)2 * (size_t)(L.maxWindow + L.n) + (size_t)(L.n + L.maxLookahead)) * sizeof(float);
		hipLaunchKernelGGL(LimiterStageKernel, dim3((unsigned)L.count), dim3(kLimThreads), lds, stream, L);
		limLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long LimiterStageLaunches() { return limLaunches.load(std::memory_order_relaxed); }
}
