// eq_stage_kernels.hip -- the device side of the EQ stage (eq_stage.h): ONE launch per processing call with entries,
// over a table of the streams with an entry only.  No reference counterpart (its hosts run their biquads on the CPU).
//
// A biquad cascade is serial in time but not across sections: section i can work on sample t - i while section i + 1 works on sample
// t - i - 1.  So the cascade runs as a PIPELINE ACROSS LANES.  A workgroup is one wave; a 16-lane DPP row is one entry; lanes 0 .. 7 of
// the row are the sections of the cascade the stream has (fades to), lanes 8 .. 15 those of the cascade it fades from, so a wave holds
// four entries.  In step t lane i of a half takes what lane i - 1 produced in step t - 1 (DPP row_shr:1, an f64 as two 32-bit moves; lane 0
// of a half takes the row's sample t, sanitised and widened), runs ITS section's step on it (EqSectionStep: the one step function of
// both sides, contraction off) and keeps the result for lane i + 1.  A lane beyond the cascade's sections passes its input on, so
// every cascade is 8 lanes deep and its output leaves lane 7 of its half, 7 steps behind its input.  Each section performs the same
// separately rounded operations in the same order on the same operands as the sequential loop: the bits are the same.
//
// Rows move through an LDS tile of 4 entries x 128 samples the way GateDetectKernel's do -- row by row, neighbouring lanes on
// neighbouring samples, so global accesses are coalesced -- with an odd row stride.  The pipeline drains at the end of every tile (7 steps
// in 135), so that every lane's section has seen exactly the tile's samples and the states in registers are those of the sequential
// loop; they are stored once at the end of the call.  The outputs of the two halves go to two tiles, and the fade's weighted sum is
// taken on the way out, a sample per lane, off the serial chain.  Rows are read and written sample by sample whatever their alignment:
// one path, so alignment and stride cannot show in the bits.  What a launch costs is one wave's chain of n + 7 * tiles steps of five
// dependent f64 operations; a lane-per-entry kernel, serial over the sections, would have a chain 8 times as long at 8 sections.
#include <hip/hip_runtime.h>

#include <atomic>

#include "eq_stage.h"

namespace na
{
	namespace
	{
		constexpr int kEqLanes = 64;          // one wave
		constexpr int kEqRowLanes = 16;       // a DPP row: one entry
		constexpr int kEqEntries = kEqLanes / kEqRowLanes; // entries of one workgroup
		constexpr int kEqTileSamples = 128;
		constexpr int kEqTileStride = kEqTileSamples + 1; // (odd: the rows start on different banks)
		constexpr int kEqDepth = kEqMaxSections;          // lanes of a cascade
		std::atomic<unsigned long long> eqLaunches{ 0 };
		static_assert(kEqRowLanes == 2 * kEqMaxSections, "a DPP row holds the two cascades of a fade");

		// what lane - 1 of the same DPP row holds (row_shr:1; lane 0 of a row reads zero): an f64 as two 32-bit moves
		__device__ __forceinline__ double EqFromLeft(double v)
		{
			const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
			const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(bits & 0xffffffffull), 0x111, 0xf, 0xf, true);
			const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(bits >> 32), 0x111, 0xf, 0xf, true);
			return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
		}
	}

	__global__ __launch_bounds__(kEqLanes) void EqStageKernel(const EqLaunch L)
	{
		__shared__ float tileTo[kEqEntries * kEqTileStride];   // in: the rows' samples; out: the outputs of the `to` cascades, in place
		__shared__ float tileFrom[kEqEntries * kEqTileStride]; // out: the outputs of the `from` cascades of fading entries
		__shared__ int rowOf[kEqEntries], fadeN[kEqEntries], fadeK[kEqEntries];
		const int lane = threadIdx.x;
		const int r = lane / kEqRowLanes;          // the entry of this workgroup the lane works for
		const int half = (lane / kEqDepth) & 1;    // 0: the cascade the stream has (fades to), 1: the one it fades from
		const int i = lane % kEqDepth;             // the lane's section
		const int first = blockIdx.x * kEqEntries;
		const int here = min(kEqEntries, L.count - first); // entries of this workgroup
		bool runs = false;                         // the lane's half is a cascade of this call
		bool mine = false;                         // ... and the lane one of its sections
		EqSection c;
		EqSecState s;
		int slot = 0;
		long long row = -1;
		if (r < here)
		{
			const EqEntry e = L.table[first + r];
			row = e.row;
			runs = half == 0 || e.fading != 0;
			slot = half == 0 ? e.slotTo : 1 - e.slotTo;
			const int S = half == 0 ? e.STo : e.SFrom;
			mine = runs && i < S;
			if (mine)
			{
				// the coefficients: the slot's own, or -- the first call after a set call -- the set that came with the table, filed into the slot
				const int set = half == 0 ? e.coefTo : e.coefFrom;
				EqSection* own = &L.coefs[row * 2 + slot].s[i];
				if (set >= 0)
				{
					c = reinterpret_cast<const EqCoefSet*>(L.table + L.count)[set].s[i];
					*own = c;
				}
				else c = *own;
				// the states: sections [0, keep) of the slot they are read from, zero beyond
				const int src = half == 0 ? e.srcTo : slot;
				const int keep = half == 0 ? e.keepTo : e.keepFrom;
				if (i < keep) s = L.state[(row * 2 + src) * kEqMaxSections + i];
			}
			if (lane % kEqRowLanes == 0)
			{
				rowOf[r] = e.row;
				fadeN[r] = e.fading ? e.N : 0;
				fadeK[r] = e.fk;
			}
		}
		__syncthreads(); // (every state is read before any is written: the `to` half may start from the `from` slot's)
		float* out = (half == 0 ? tileTo : tileFrom) + r * kEqTileStride;
		const float* in = tileTo + r * kEqTileStride;
		for (unsigned long long t0 = 0; t0 < L.n; t0 += kEqTileSamples)
		{
			const int len = (int)min((unsigned long long)kEqTileSamples, L.n - t0);
			// in: row q of the tile is entry q's row, lanes along the samples
			for (int q = 0; q < here; q++)
			{
				const float* src = L.rows + (long long)rowOf[q] * L.stride + t0;
				for (int j = lane; j < len; j += kEqLanes) tileTo[q * kEqTileStride + j] = src[j];
			}
			__syncthreads();
			double v = 0.0;
			float x = in[0];
			for (int step = 0; step < len + kEqDepth - 1; step++)
			{
				double vin = EqFromLeft(v); // (all 64 lanes: the DPP move is outside every branch)
				if (i == 0) vin = (double)EqSanitize(x);
				x = in[min(step + 1, len - 1)]; // (the next step's sample, read ahead of this step's chain; outputs trail the reads by 7)
				const int t = step - i;       // the sample of the tile this lane works on
				if (runs && t >= 0 && t < len)
				{
					v = mine ? EqSectionStep(c, s, vin) : vin;
					if (i == kEqDepth - 1) out[t] = (float)v;
				}
			}
			__syncthreads();
			// out: the way the samples came; a fading entry's sample is the weighted sum of its two cascades' outputs
			for (int q = 0; q < here; q++)
			{
				float* dst = L.rows + (long long)rowOf[q] * L.stride + t0;
				const int N = fadeN[q];
				const long long k0 = (long long)fadeK[q] + (long long)t0;
				for (int j = lane; j < len; j += kEqLanes)
				{
					float o = tileTo[q * kEqTileStride + j];
					if (N > 0) o = EqMix(N, k0 + j, tileFrom[q * kEqTileStride + j], o);
					dst[j] = o;
				}
			}
			__syncthreads();
		}
		if (mine) L.state[(row * 2 + slot) * kEqMaxSections + i] = s;
	}

	hipError_t LaunchEqStage(const EqLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n == 0) return hipSuccess;
		if (!L.table || !L.rows || !L.coefs || !L.state) return hipErrorInvalidValue;
		hipLaunchKernelGGL(EqStageKernel, dim3((unsigned)((L.count + kEqEntries - 1) / kEqEntries)), dim3(kEqLanes), 0, stream, L);
		eqLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long EqStageLaunches() { return eqLaunches.load(std::memory_order_relaxed); }
}
