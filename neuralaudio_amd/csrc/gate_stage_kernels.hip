// gate_stage_kernels.hip -- the device side of the gate stage (gate_stage.h): TWO launches per processing call with
// entries, over a table of the gated streams only.  No reference counterpart (its hosts gate on the CPU).
//
// Detector, in front of the model launches.  The recurrence is strictly serial per stream, so the only parallelism is across entries:
// one lane per entry, 64 entries to a workgroup of one wave.  A lane walking along its own row would make every global access of the
// wave 64 separate rows; instead the wave moves a tile of 64 entries x 128 samples through LDS -- row by row, neighbouring lanes on
// neighbouring samples, so global loads and stores are coalesced -- and each lane then walks ITS row of the tile.  The tile's row stride
// is 129 floats: lane e reads word e * 129 + j, so the 64 lanes fall on 64 different banks.  The state stays in registers across the
// tiles of a call and is stored once at the end; the gains replace the samples in the tile and leave the same way they came.  Rows are
// read sample by sample whatever their alignment: there is one path, so alignment and stride cannot show in the bits.  What a launch
// costs is one wave's dependent chain over n samples.
//
// Apply, behind the model launches: y *= g on the entries' rows, shaped like OutputStageKernel -- one workgroup column per entry, one
// wave per 256 samples, float4 where rows and strides are 16-byte aligned, sample by sample elsewhere; both paths do the same single
// multiplication.  Rows without an entry are never touched.
#include <hip/hip_runtime.h>

#include <atomic>

#include "gate_stage.h"

namespace na
{
	namespace
	{
		constexpr int kGateLanes = 64;        // entries of one workgroup (one wave)
		constexpr int kGateTileSamples = 128; // samples of a tile
		constexpr int kGateTileStride = kGateTileSamples + 1; // (odd: the lanes' rows start on different banks)
		constexpr int kGateApplyThreads = 64;
		constexpr int kGateApplySamplesPerBlock = 256; // a wave of float4
		std::atomic<unsigned long long> gateLaunches{ 0 };
	}

	__global__ __launch_bounds__(kGateLanes) void GateDetectKernel(const GateDetectLaunch L)
	{
		__shared__ float tile[kGateLanes * kGateTileStride];
		__shared__ int rowOf[kGateLanes];
		const int lane = threadIdx.x;
		const int first = blockIdx.x * kGateLanes;
		const int here = min(kGateLanes, L.count - first); // entries of this workgroup
		const bool mine = lane < here;
		GateEntry e;
		GateState s;
		if (mine)
		{
			e = L.table[first + lane];
			s = GateBegin(e, L.state[e.row]);
		}
		rowOf[lane] = mine ? e.row : -1;
		__syncthreads();
		for (unsigned long long t0 = 0; t0 < L.n; t0 += kGateTileSamples)
		{
			const int len = (int)min((unsigned long long)kGateTileSamples, L.n - t0);
			// in: row r of the tile is entry r's input, lanes along the samples
			for (int r = 0; r < here; r++)
			{
				const float* src = L.in + (long long)rowOf[r] * L.inStride + t0;
				for (int j = lane; j < len; j += kGateLanes) tile[r * kGateTileStride + j] = src[j];
			}
			__syncthreads();
			if (mine)
			{
				float* my = tile + lane * kGateTileStride;
				for (int j = 0; j < len; j++) my[j] = GateStep(e.c, e.forceOpen, s, my[j]);
			}
			__syncthreads();
			// out: the gains, the way the samples came
			for (int r = 0; r < here; r++)
			{
				float* dst = L.gains + (long long)rowOf[r] * L.gainSamples + t0;
				for (int j = lane; j < len; j += kGateLanes) dst[j] = tile[r * kGateTileStride + j];
			}
			__syncthreads();
		}
		if (mine) L.state[e.row] = s;
	}

	template <bool VEC>
	__global__ __launch_bounds__(kGateApplyThreads) void GateApplyKernel(const GateApplyLaunch L)
	{
		const int row = L.table[blockIdx.x].row;
		if (row < 0) return;
		float* __restrict__ y = L.rows + (long long)row * L.stride;
		const float* __restrict__ g = L.gains + (long long)row * L.gainSamples;
		const unsigned long long blocks = (L.n + kGateApplySamplesPerBlock - 1) / kGateApplySamplesPerBlock;
		for (unsigned long long blk = blockIdx.y; blk < blocks; blk += gridDim.y)
		{
			const unsigned long long base = blk * kGateApplySamplesPerBlock;
			if (VEC)
			{
				const unsigned long long i = base + 4ull * threadIdx.x;
				if (i + 4 <= L.n)
				{
					float4 v = *reinterpret_cast<const float4*>(y + i);
					const float4 w = *reinterpret_cast<const float4*>(g + i); // (gain rows are 16-byte aligned: gainSamples is a power of two)
					v.x *= w.x;
					v.y *= w.y;
					v.z *= w.z;
					v.w *= w.w;
					*reinterpret_cast<float4*>(y + i) = v;
				}
				else
				{
					// (the last, partial vector of the row)
					for (unsigned long long j = i; j < L.n; j++) y[j] *= g[j];
				}
			}
			else
			{
				for (int q = 0; q < kGateApplySamplesPerBlock / kGateApplyThreads; q++)
				{
					const unsigned long long j = base + (unsigned long long)q * kGateApplyThreads + threadIdx.x; // (neighbouring lanes, neighbouring samples)
					if (j >= L.n) break;
					y[j] *= g[j];
				}
			}
		}
	}

	hipError_t LaunchGateDetect(const GateDetectLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.in || !L.gains || !L.state || L.n > (unsigned long long)L.gainSamples) return hipErrorInvalidValue;
		hipLaunchKernelGGL(GateDetectKernel, dim3((unsigned)((L.count + kGateLanes - 1) / kGateLanes)), dim3(kGateLanes), 0, stream, L);
		gateLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	hipError_t LaunchGateApply(const GateApplyLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rows || !L.gains || L.n > (unsigned long long)L.gainSamples) return hipErrorInvalidValue;
		const unsigned long long blocks = (L.n + kGateApplySamplesPerBlock - 1) / kGateApplySamplesPerBlock;
		const dim3 grid((unsigned)L.count, (unsigned)std::min<unsigned long long>(blocks, 1024ull));
		const bool vec = (reinterpret_cast<uintptr_t>(L.rows) % 16 == 0) && (L.stride % 4 == 0);
		if (vec) hipLaunchKernelGGL(GateApplyKernel<true>, grid, dim3(kGateApplyThreads), 0, stream, L);
		else hipLaunchKernelGGL(GateApplyKernel<false>, grid, dim3(kGateApplyThreads), 0, stream, L);
		gateLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long GateStageLaunches() { return gateLaunches.load(std::memory_order_relaxed); }
}
