// compressor_stage_kernels.hip -- the device side of the compressor stage (compressor_stage.h): ONE launch per
// processing call with entries, over a table of the compressed streams only.  No reference counterpart (its hosts run their dynamics
// on the CPU).
//
// The only serial code of the stage is the level follower: three dependent f32 operations and a select per sample and stream.
// Everything behind it -- the curve reads, the fade, the multiplication -- depends on the follower's value at that sample alone and is
// sample-parallel.  The gate's detector and the delay's line run ALL of their work on one wave that stages 64 rows through LDS by
// itself, and what they cost is that wave's latency (profiles/gate_cost.txt, profiles/delay_cost.txt).  Here a workgroup of four waves
// owns 16 entries, so 1024 entries are 64 workgroups, and walks the call in tiles of 128 samples in three phases:
//   A  all four waves, lanes along the samples: coalesced loads of the group's rows, x' = CompLevel(x) into an LDS tile (row stride
//      129 floats: the 16 lanes of phase B fall on 16 different banks); every thread keeps the eight samples it loaded in registers
//   B  one wave, one lane per entry: walks ITS row of the tile and replaces x' by e (CompFollow); e stays in a register across the
//      tiles of a call and is stored once
//   C  all four waves, lanes along the samples again, every thread on the samples it loaded: the curves at e (CompCurveAt: the lanes of
//      a row read neighbouring knots of one 2 KB curve, a gather that L1 / L2 serve), the fade's weight from the sample's integer
//      position, g (CompGain), y = x * g, coalesced store in place
// Rows are read and written sample by sample whatever their alignment: one path, so alignment and stride cannot show in the bits.
// A curve that came with the table is read from the table in this call and filed into the row's slot for the calls after it.
#include <hip/hip_runtime.h>

#include <atomic>

#include "compressor_stage.h"

namespace na
{
	namespace
	{
		constexpr int kCompThreads = 256;      // four waves
		constexpr int kCompTileSamples = 128;  // samples of a tile
		constexpr int kCompTileStride = kCompTileSamples + 1; // (odd: the lanes' rows start on different banks)
		constexpr int kCompPerThread = kCompGroupEntries * kCompTileSamples / kCompThreads; // samples of a tile a thread owns: 8
		constexpr int kCompRowStep = kCompThreads / kCompTileSamples;                       // ... in rows this far apart: 2
		std::atomic<unsigned long long> compLaunches{ 0 };
		static_assert(kCompThreads % kCompTileSamples == 0 && kCompPerThread * kCompRowStep == kCompGroupEntries, "a thread owns one column of every second row");
	}

	__global__ __launch_bounds__(kCompThreads) void CompressorStageKernel(const CompLaunch L)
	{
		__shared__ float tile[kCompGroupEntries * kCompTileStride];
		__shared__ long long rowOf[kCompGroupEntries];
		__shared__ const float* curveTo[kCompGroupEntries];   // nullptr: the unity curve
		__shared__ const float* curveFrom[kCompGroupEntries];
		__shared__ int fadeN[kCompGroupEntries], fadeK[kCompGroupEntries]; // N = 0: no fade
		const int tid = threadIdx.x;
		const int first = blockIdx.x * kCompGroupEntries;
		const int here = min(kCompGroupEntries, L.count - first); // entries of this workgroup
		const float* const travelled = reinterpret_cast<const float*>(L.table + L.count); // the curves behind the entries
		float e = 0.0f, aA = 1.0f, aR = 1.0f;
		if (tid < here)
		{
			const CompEntry en = L.table[first + tid];
			rowOf[tid] = en.row;
			aA = en.aA;
			aR = en.aR;
			e = en.start ? 0.0f : L.state[en.row].e;
			const float* slotTo = L.curves[(long long)en.row * 2 + en.slotTo].t;
			const float* slotFrom = L.curves[(long long)en.row * 2 + (1 - en.slotTo)].t;
			curveTo[tid] = en.unityTo ? nullptr : (en.coefTo >= 0 ? travelled + (long long)en.coefTo * kCompCurveFloats : slotTo);
			curveFrom[tid] = en.unityFrom ? nullptr : (en.coefFrom >= 0 ? travelled + (long long)en.coefFrom * kCompCurveFloats : slotFrom);
			fadeN[tid] = en.fading ? en.N : 0;
			fadeK[tid] = en.fk;
		}
		// the curves that came with the table go into their slots (nothing of this launch reads them there)
		for (int r = 0; r < here; r++)
		{
			const CompEntry en = L.table[first + r];
			if (en.coefTo >= 0)
			{
				float* dst = L.curves[(long long)en.row * 2 + en.slotTo].t;
				const float* src = travelled + (long long)en.coefTo * kCompCurveFloats;
				for (int i = tid; i < kCompCurvePoints; i += kCompThreads) dst[i] = src[i];
			}
			if (en.coefFrom >= 0)
			{
				float* dst = L.curves[(long long)en.row * 2 + (1 - en.slotTo)].t;
				const float* src = travelled + (long long)en.coefFrom * kCompCurveFloats;
				for (int i = tid; i < kCompCurvePoints; i += kCompThreads) dst[i] = src[i];
			}
		}
		__syncthreads();
		const int j = tid % kCompTileSamples;     // the thread's column of the tile
		const int r0 = tid / kCompTileSamples;    // ... and its first row
		for (unsigned long long t0 = 0; t0 < L.n; t0 += kCompTileSamples)
		{
			const int len = (int)min((unsigned long long)kCompTileSamples, L.n - t0);
			float x[kCompPerThread];
			// A
#pragma unroll
			for (int q = 0; q < kCompPerThread; q++)
			{
				const int r = q * kCompRowStep + r0;
				x[q] = 0.0f;
				if (r < here && j < len)
				{
					x[q] = L.rows[rowOf[r] * L.stride + (long long)t0 + j];
					tile[r * kCompTileStride + j] = CompLevel(x[q]);
				}
			}
			__syncthreads();
			// B
			if (tid < here)
			{
				float* my = tile + tid * kCompTileStride;
				for (int s = 0; s < len; s++)
				{
					e = CompFollow(aA, aR, e, my[s]);
					my[s] = e;
				}
			}
			__syncthreads();
			// C
#pragma unroll
			for (int q = 0; q < kCompPerThread; q++)
			{
				const int r = q * kCompRowStep + r0;
				if (r < here && j < len)
				{
					const float level = tile[r * kCompTileStride + j];
					const float* tB = curveTo[r];
					const float gB = tB ? CompCurveAt(tB, level) : 1.0f;
					float g = gB;
					const int N = fadeN[r];
					if (N > 0)
					{
						const float w = OutStageWeightAt(N, (long long)fadeK[r] + (long long)t0 + j);
						if (w != 1.0f)
						{
							const float* tA = curveFrom[r];
							g = CompGain(w, tA ? CompCurveAt(tA, level) : 1.0f, gB);
						}
					}
					L.rows[rowOf[r] * L.stride + (long long)t0 + j] = x[q] * g;
					if (t0 + (unsigned long long)j + 1 == L.n) L.state[rowOf[r]].g = g;
				}
			}
			__syncthreads(); // (the next tile's phase A writes where this one's phase C read)
		}
		if (tid < here) L.state[rowOf[tid]].e = e;
	}

	hipError_t LaunchCompressorStage(const CompLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rows || !L.curves || !L.state) return hipErrorInvalidValue;
		hipLaunchKernelGGL(CompressorStageKernel, dim3((unsigned)((L.count + kCompGroupEntries - 1) / kCompGroupEntries)), dim3(kCompThreads), 0, stream, L);
		compLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long CompressorStageLaunches() { return compLaunches.load(std::memory_order_relaxed); }
}
