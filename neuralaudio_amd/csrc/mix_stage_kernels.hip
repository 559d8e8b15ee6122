// mix_stage_kernels.hip -- the device side of the mix stage (mix_stage.h): ONE launch per processing call with groups,
// behind the output stage, over a table of the groups only -- and, where a group has a DRY member, one small launch in front of the
// models that keeps those streams' input rows (they may be the memory the models write).  No reference counterpart (its hosts sum on
// the CPU).
//
// Shape of the work: the output stage's -- a short memory-bound pass whose cost is its launch.  One workgroup column per group
// (blockIdx.x), one wave per 256 samples of it (blockIdx.y); rows and strides that are 16-byte aligned move as float4, everything else
// sample by sample, and both paths do the same arithmetic on every sample (MixGainOf / MixAccumulate: the step functions of both sides,
// contraction off), so the path never shows in the output.  The thread that owns a sample position reads that sample from all M
// sources into registers before it writes any of the D outputs: an output row that is a source of a later output is read raw, and no
// entry, wave or launch ever sees a half-mixed group.  The two matrices sit in LDS, read at wave-uniform addresses; a call that the
// ramp does not reach (k >= R - 1 from its first sample) takes a branch with constant gains and no ramp arithmetic.  Rows that are no
// output of a group are never written.
#include <hip/hip_runtime.h>

#include <atomic>

#include "mix_stage.h"

namespace na
{
	namespace
	{
		constexpr int kMixThreads = 64;
		constexpr int kMixSamplesPerBlock = 256; // a wave of float4
		std::atomic<unsigned long long> mixLaunches{ 0 }, stashLaunches{ 0 };

		// what one group's workgroup works with: the matrices and the output rows in LDS, the members' sources
		struct MixGroupView
		{
			const float* G;                     // LDS: g0 [8][8], then g1 [8][8]
			const int* outRow;                  // LDS: the rows of the members
			const float* src[kMixMaxMembers];   // member j's row: the output row, or the stashed input row
			int M, D, R, k;
		};

		// output d of the sample at ramp position `pos` from the sample's M sources
		template <bool FLAT>
		__device__ __forceinline__ float MixOutput(const MixGroupView& v, int d, long long pos, const float (&y)[kMixMaxMembers])
		{
			const bool reached = FLAT || pos >= (long long)v.R - 1;
			const float w = reached ? 1.0f : MixWeightAt(v.R, pos);
			float acc = 0.0f;
			bool any = false;
#pragma unroll
			for (int j = 0; j < kMixMaxMembers; j++)
			{
				if (j >= v.M) continue;
				const int c = d * kMixMaxMembers + j;
				const float g = reached ? v.G[kMixMatrixFloats + c] : MixGainOf(v.G[c], v.G[kMixMatrixFloats + c], w);
				MixAccumulate(acc, any, g, y[j]);
			}
			return any ? acc : 0.0f;
		}

		// one sample position, sample by sample: every source first, then every output
		template <bool FLAT>
		__device__ __forceinline__ void MixOne(const MixGroupView& v, float* rows, long stride, unsigned long long i)
		{
			float y[kMixMaxMembers];
#pragma unroll
			for (int j = 0; j < kMixMaxMembers; j++) y[j] = j < v.M ? v.src[j][i] : 0.0f;
#pragma unroll 1
			for (int d = 0; d < v.D; d++) rows[(long long)v.outRow[d] * stride + (long long)i] = MixOutput<FLAT>(v, d, (long long)v.k + (long long)i, y);
		}

		template <bool VEC, bool FLAT>
		__device__ __forceinline__ void MixRun(const MixGroupView& v, float* rows, long stride, unsigned long long n)
		{
			const unsigned long long blocks = (n + kMixSamplesPerBlock - 1) / kMixSamplesPerBlock;
			for (unsigned long long blk = blockIdx.y; blk < blocks; blk += gridDim.y)
			{
				const unsigned long long base = blk * kMixSamplesPerBlock;
				if (VEC)
				{
					const unsigned long long i = base + 4ull * threadIdx.x;
					if (i + 4 <= n)
					{
						float y[4][kMixMaxMembers];
#pragma unroll
						for (int j = 0; j < kMixMaxMembers; j++)
						{
							float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
							if (j < v.M) t = *reinterpret_cast<const float4*>(v.src[j] + i);
							y[0][j] = t.x;
							y[1][j] = t.y;
							y[2][j] = t.z;
							y[3][j] = t.w;
						}
						const long long pos = (long long)v.k + (long long)i;
#pragma unroll 1
						for (int d = 0; d < v.D; d++)
						{
							float4 o;
							o.x = MixOutput<FLAT>(v, d, pos + 0, y[0]);
							o.y = MixOutput<FLAT>(v, d, pos + 1, y[1]);
							o.z = MixOutput<FLAT>(v, d, pos + 2, y[2]);
							o.w = MixOutput<FLAT>(v, d, pos + 3, y[3]);
							*reinterpret_cast<float4*>(rows + (long long)v.outRow[d] * stride + (long long)i) = o;
						}
					}
					else
					{
						// (the last, partial vector of the row)
						for (unsigned long long j = i; j < n; j++) MixOne<FLAT>(v, rows, stride, j);
					}
				}
				else
				{
					for (int q = 0; q < kMixSamplesPerBlock / kMixThreads; q++)
					{
						const unsigned long long j = base + (unsigned long long)q * kMixThreads + threadIdx.x; // (neighbouring lanes, neighbouring samples)
						if (j >= n) break;
						MixOne<FLAT>(v, rows, stride, j);
					}
				}
			}
		}
	}

	template <bool VEC>
	__global__ __launch_bounds__(kMixThreads) void MixStageKernel(const MixLaunch L)
	{
		__shared__ float G[kMixSetFloats];
		__shared__ int outRow[kMixMaxMembers];
		const MixEntry e = L.table[blockIdx.x];
		if (e.M <= 0 || e.M > kMixMaxMembers || e.D <= 0 || e.D > e.M) return;
		// the matrices: the block's own, or -- the first call after a set call -- the set that came with the table, filed into the block
		// by the group's first workgroup (no other workgroup of this launch reads the block's copy)
		float* own = L.gains + (long long)e.row[0] * kMixSetFloats;
		const float* from = e.gainSet >= 0 ? reinterpret_cast<const float*>(L.table + L.count + (long long)e.gainSet * kMixSetEntries) : own;
		for (int c = threadIdx.x; c < kMixSetFloats; c += kMixThreads)
		{
			const float g = from[c];
			G[c] = g;
			if (e.gainSet >= 0 && blockIdx.y == 0) own[c] = g;
		}
		if (threadIdx.x < kMixMaxMembers) outRow[threadIdx.x] = L.table[blockIdx.x].row[threadIdx.x]; // (from memory: a lane-indexed read of `e` would move it out of the scalar registers)
		__syncthreads();
		MixGroupView v;
		v.G = G;
		v.outRow = outRow;
		v.M = e.M;
		v.D = e.D;
		v.R = e.R;
		v.k = e.k;
#pragma unroll
		for (int j = 0; j < kMixMaxMembers; j++)
		{
			const int row = j < e.M ? e.row[j] : e.row[0];
			const bool dry = j < e.M && ((e.dryMask >> j) & 1) != 0;
			v.src[j] = dry ? L.stash + (long long)row * L.drySamples : L.rows + (long long)row * L.stride;
		}
		if ((long long)e.k >= (long long)e.R - 1) MixRun<VEC, true>(v, L.rows, L.stride, L.n);
		else MixRun<VEC, false>(v, L.rows, L.stride, L.n);
	}

	// the input rows of the DRY members, as the caller passed them, into the stage's block: sample by sample whatever the alignment
	__global__ __launch_bounds__(kMixThreads) void MixStashKernel(const MixStashLaunch L)
	{
		const MixEntry e = L.table[blockIdx.x];
		if (e.dryMask == 0 || e.M <= 0 || e.M > kMixMaxMembers) return;
		const unsigned long long blocks = (L.n + kMixSamplesPerBlock - 1) / kMixSamplesPerBlock;
		for (unsigned long long blk = blockIdx.y; blk < blocks; blk += gridDim.y)
			for (int q = 0; q < kMixSamplesPerBlock / kMixThreads; q++)
			{
				const unsigned long long i = blk * kMixSamplesPerBlock + (unsigned long long)q * kMixThreads + threadIdx.x;
				if (i >= L.n) break;
#pragma unroll
				for (int j = 0; j < kMixMaxMembers; j++)
					if (j < e.M && ((e.dryMask >> j) & 1) != 0) L.stash[(long long)e.row[j] * L.drySamples + (long long)i] = L.in[(long long)e.row[j] * L.inStride + (long long)i];
			}
	}

	hipError_t LaunchMixStage(const MixLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rows || !L.gains) return hipErrorInvalidValue;
		const unsigned long long blocks = (L.n + kMixSamplesPerBlock - 1) / kMixSamplesPerBlock;
		const dim3 grid((unsigned)L.count, (unsigned)std::min<unsigned long long>(blocks, 1024ull));
		// (the stash block is 16-byte aligned and its rows a power of two >= 2048 floats apart: it never decides the path)
		const bool vec = (reinterpret_cast<uintptr_t>(L.rows) % 16 == 0) && (L.stride % 4 == 0);
		if (vec) hipLaunchKernelGGL(MixStageKernel<true>, grid, dim3(kMixThreads), 0, stream, L);
		else hipLaunchKernelGGL(MixStageKernel<false>, grid, dim3(kMixThreads), 0, stream, L);
		mixLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	hipError_t LaunchMixStash(const MixStashLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.in || !L.stash || L.n > (unsigned long long)L.drySamples) return hipErrorInvalidValue;
		const unsigned long long blocks = (L.n + kMixSamplesPerBlock - 1) / kMixSamplesPerBlock;
		const dim3 grid((unsigned)L.count, (unsigned)std::min<unsigned long long>(blocks, 1024ull));
		hipLaunchKernelGGL(MixStashKernel, grid, dim3(kMixThreads), 0, stream, L);
		stashLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long MixStageLaunches() { return mixLaunches.load(std::memory_order_relaxed); }
	unsigned long long MixStashLaunches() { return stashLaunches.load(std::memory_order_relaxed); }
}
