// output_stage_kernels.hip -- the device side of the output stage (output_stage.h): ONE launch per buffer behind the
// model launches, over a table of active entries only.  No reference counterpart (its hosts scale and cross-fade on the CPU).
//
// Shape of the work: a short memory-bound pass, 2 x 512 bytes per entry at 128 samples -- what it costs is its launch.  One workgroup
// column per entry (blockIdx.x), one wave per 256 samples of it (blockIdx.y); rows and strides that are 16-byte aligned move as float4,
// everything else sample by sample, and both paths do the same arithmetic on every sample, so the path never shows in the output.  A fade
// pair is one entry: the thread that owns a sample reads it from both raw rows before it writes either, so no other entry, wave or
// launch ever sees a half-updated pair.  Rows without an entry are never touched.
#include <hip/hip_runtime.h>

#include "output_stage.h"

namespace na
{
	namespace
	{
		constexpr int kOutStageThreads = 64;
		constexpr int kOutStageSamplesPerBlock = 256; // a wave of float4

		// sample `i` of the call: both rows' new values from both raw values
		__device__ __forceinline__ void OutStageSample(const OutStageEntry& e, long long i, float yA, float yB, float& outA, float& outB)
		{
			const float a = OutStageGainAt(e.a, (long long)e.a.k + i) * yA;
			outA = a;
			if (e.rowB < 0) return;
			const float b = OutStageGainAt(e.b, (long long)e.b.k + i) * yB;
			const float w = OutStageWeightAt(e.N, (long long)e.fk + i);
			outB = (1.0f - w) * a + w * b;
		}
	}

	template <bool VEC>
	__global__ __launch_bounds__(kOutStageThreads) void OutputStageKernel(const OutStageLaunch L)
	{
		const OutStageEntry e = L.table[blockIdx.x];
		if (e.rowA < 0) return;
		const bool pair = e.rowB >= 0;
		float* __restrict__ rowA = L.rows + (long long)e.rowA * L.stride;
		float* rowB = pair ? L.rows + (long long)e.rowB * L.stride : rowA;
		const unsigned long long blocks = (L.n + kOutStageSamplesPerBlock - 1) / kOutStageSamplesPerBlock;
		for (unsigned long long blk = blockIdx.y; blk < blocks; blk += gridDim.y)
		{
			const unsigned long long base = blk * kOutStageSamplesPerBlock;
			if (VEC)
			{
				const unsigned long long i = base + 4ull * threadIdx.x;
				if (i + 4 <= L.n)
				{
					const float4 yA = *reinterpret_cast<const float4*>(rowA + i);
					float4 yB = yA;
					if (pair) yB = *reinterpret_cast<const float4*>(rowB + i);
					float4 oA, oB = yB;
					OutStageSample(e, (long long)i + 0, yA.x, yB.x, oA.x, oB.x);
					OutStageSample(e, (long long)i + 1, yA.y, yB.y, oA.y, oB.y);
					OutStageSample(e, (long long)i + 2, yA.z, yB.z, oA.z, oB.z);
					OutStageSample(e, (long long)i + 3, yA.w, yB.w, oA.w, oB.w);
					*reinterpret_cast<float4*>(rowA + i) = oA;
					if (pair) *reinterpret_cast<float4*>(rowB + i) = oB;
				}
				else
				{
					// (the last, partial vector of the row)
					for (unsigned long long j = i; j < L.n; j++)
					{
						const float yA = rowA[j];
						const float yB = pair ? rowB[j] : yA;
						float oA, oB = yB;
						OutStageSample(e, (long long)j, yA, yB, oA, oB);
						rowA[j] = oA;
						if (pair) rowB[j] = oB;
					}
				}
			}
			else
			{
				for (int q = 0; q < kOutStageSamplesPerBlock / kOutStageThreads; q++)
				{
					const unsigned long long j = base + (unsigned long long)q * kOutStageThreads + threadIdx.x; // (neighbouring lanes, neighbouring samples)
					if (j >= L.n) break;
					const float yA = rowA[j];
					const float yB = pair ? rowB[j] : yA;
					float oA, oB = yB;
					OutStageSample(e, (long long)j, yA, yB, oA, oB);
					rowA[j] = oA;
					if (pair) rowB[j] = oB;
				}
			}
		}
	}

	hipError_t LaunchOutputStage(const OutStageLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rows) return hipErrorInvalidValue;
		const unsigned long long blocks = (L.n + kOutStageSamplesPerBlock - 1) / kOutStageSamplesPerBlock;
		const dim3 grid((unsigned)L.count, (unsigned)std::min<unsigned long long>(blocks, 1024ull));
		const bool vec = (reinterpret_cast<uintptr_t>(L.rows) % 16 == 0) && (L.stride % 4 == 0);
		if (vec) hipLaunchKernelGGL(OutputStageKernel<true>, grid, dim3(kOutStageThreads), 0, stream, L);
		else hipLaunchKernelGGL(OutputStageKernel<false>, grid, dim3(kOutStageThreads), 0, stream, L);
		return hipGetLastError();
	}
}
