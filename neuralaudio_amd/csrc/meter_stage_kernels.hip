// meter_stage_kernels.hip -- the device side of the meter stage (meter_stage.h): TWO launches per processing call with
// entries, over a table of the metered streams only -- the IN tap in front of the model launches (the input rows may be the output
// rows), the OUT and GATE taps behind the output stage.  No reference counterpart (its hosts meter on the CPU).  Neither launch writes
// an audio row.
//
// Every quantity is a max, a min or an integer sum, so lanes go along the samples: one wave per entry, lane l takes samples l, l + 64,
// ... of a run -- neighbouring lanes on neighbouring samples, coalesced loads at any alignment through one code path, so alignment
// and stride cannot show in the bits.  The call is cut into runs at the window boundaries of the entry (MeterRunLength): a call may
// hold a fraction of a window or several windows.  The lanes' partials of a run are reduced across the wave in registers -- two
// quad permutes, a half-row and a row mirror as DPP moves, then one readlane per row of 16 -- with plain integer max / min / add; the
// 64-bit energy travels as two words and is added with its carry (MeterAdd64).  No LDS, no atomics.  Every lane then holds the run's
// partial and walks the tap's state through MeterFold alike (the state is wave-uniform); lane 0 stores the state, the published
// window and -- the OUT launch -- the entry's result record.
#include <hip/hip_runtime.h>

#include <atomic>

#include "meter_stage.h"

namespace na
{
	namespace
	{
		constexpr int kMeterLanes = 64; // one wave per entry
		std::atomic<unsigned long long> meterLaunches{ 0 };

		constexpr int kDppQuadSwap1 = 0xB1;    // quad_perm:[1,0,3,2]
		constexpr int kDppQuadSwap2 = 0x4E;    // quad_perm:[2,3,0,1]
		constexpr int kDppHalfMirror = 0x141;  // row_half_mirror
		constexpr int kDppRowMirror = 0x140;   // row_mirror

		template <int CTRL>
		__device__ __forceinline__ uint32_t DppMove(uint32_t v)
		{
			return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
		}

		template <int CTRL>
		__device__ __forceinline__ void MergeStep(MeterPartial& p, uint32_t& gmin)
		{
			MeterPartial o;
			o.peakBits = DppMove<CTRL>(p.peakBits);
			o.overs = DppMove<CTRL>(p.overs);
			o.energyLo = DppMove<CTRL>(p.energyLo);
			o.energyHi = DppMove<CTRL>(p.energyHi);
			const uint32_t og = DppMove<CTRL>(gmin);
			MeterMerge(p, o);
			gmin = min(gmin, og);
		}

		__device__ __forceinline__ uint32_t LaneValue(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

		// every lane's partial of a run -> the run's partial, in every lane.  The steps pair disjoint sets of lanes (2, 4, 8, 16 lanes hold
		// the same value afterwards), then the four rows of 16 meet through readlane.
		__device__ __forceinline__ void WaveReduce(MeterPartial& p, uint32_t& gmin)
		{
			MergeStep<kDppQuadSwap1>(p, gmin);
			MergeStep<kDppQuadSwap2>(p, gmin);
			MergeStep<kDppHalfMirror>(p, gmin);
			MergeStep<kDppRowMirror>(p, gmin);
			MeterPartial total;
			uint32_t g = kMeterNoGainBits;
			for (int row = 0; row < kMeterLanes; row += 16)
			{
				MeterPartial r;
				r.peakBits = LaneValue(p.peakBits, row);
				r.overs = LaneValue(p.overs, row);
				r.energyLo = LaneValue(p.energyLo, row);
				r.energyHi = LaneValue(p.energyHi, row);
				MeterMerge(total, r);
				g = min(g, LaneValue(gmin, row));
			}
			p = total;
			gmin = g;
		}
	}

	template <bool OUT>
	__global__ __launch_bounds__(kMeterLanes) void MeterTapKernel(const MeterLaunch L)
	{
		const int lane = threadIdx.x;
		const MeterEntry e = L.table[blockIdx.x];
		if (e.row < 0 || e.window < kMeterMinWindow) return;
		MeterState* st = L.state + e.row;
		MeterTapState s = MeterBegin(e, OUT ? st->out : st->in);
		uint32_t gateMin = (OUT && e.start != kMeterStartFresh) ? st->gateMinBits : kMeterNoGainBits;
		const uint32_t W = (uint32_t)e.window;
		const uint32_t clipBits = OUT ? e.clipOutBits : e.clipInBits;
		const float* __restrict__ x = L.rows + (long long)e.row * L.stride;
		const float* __restrict__ g = (OUT && e.gated && L.gains) ? L.gains + (long long)e.row * L.gainSamples : nullptr;
		MeterTapReading pub;
		bool published = false;
		uint32_t pubGateMin = kMeterOneBits, pubGateLast = kMeterOneBits;
		for (unsigned long long i = 0; i < L.n;)
		{
			const uint32_t len = MeterRunLength(s.pos, W, L.n - i);
			MeterPartial p;
			uint32_t gmin = kMeterNoGainBits;
			for (uint32_t j = (uint32_t)lane; j < len; j += kMeterLanes)
			{
				MeterSample(p, x[i + j], clipBits);
				if (OUT) gmin = min(gmin, g ? MeterBits(g[i + j]) : kMeterOneBits);
			}
			WaveReduce(p, gmin);
			if (OUT) gateMin = min(gateMin, gmin);
			if (MeterFold(s, p, len, W, pub))
			{
				published = true;
				if (OUT)
				{
					pubGateMin = gateMin;
					pubGateLast = g ? MeterBits(g[i + len - 1]) : kMeterOneBits;
					gateMin = kMeterNoGainBits;
				}
			}
			i += len;
		}
		if (lane != 0) return;
		if (!OUT)
		{
			st->in = s;
			if (published) st->latest.in = pub;
			return;
		}
		st->out = s;
		st->gateMinBits = gateMin;
		st->gen = e.gen;
		if (published)
		{
			st->latest.out = pub;
			st->latest.gateGainMin = MeterFloat(pubGateMin);
			st->latest.gateGainLast = MeterFloat(pubGateLast);
		}
		st->latest.windows = s.windows; // (0 behind a start: nothing of an earlier meter is left to read)
		st->latest.windowSamples = e.window;
		st->latest.reserved = 0;
		MeterRecord rec;
		rec.row = e.row;
		rec.gen = e.gen;
		rec.reading = st->latest;
		L.results[blockIdx.x] = rec;
	}

	namespace
	{
		hipError_t LaunchTap(const MeterLaunch& L, bool out, hipStream_t stream)
		{
			if (L.count <= 0 || L.n == 0) return hipSuccess;
			if (!L.table || !L.rows || !L.state || (out && !L.results)) return hipErrorInvalidValue;
			if (L.gains && L.n > (unsigned long long)L.gainSamples) return hipErrorInvalidValue;
			if (out) hipLaunchKernelGGL(MeterTapKernel<true>, dim3((unsigned)L.count), dim3(kMeterLanes), 0, stream, L);
			else hipLaunchKernelGGL(MeterTapKernel<false>, dim3((unsigned)L.count), dim3(kMeterLanes), 0, stream, L);
			meterLaunches.fetch_add(1, std::memory_order_relaxed);
			return hipGetLastError();
		}
	}

	hipError_t LaunchMeterIn(const MeterLaunch& L, hipStream_t stream) { return LaunchTap(L, false, stream); }
	hipError_t LaunchMeterOut(const MeterLaunch& L, hipStream_t stream) { return LaunchTap(L, true, stream); }

	unsigned long long MeterStageLaunches() { return meterLaunches.load(std::memory_order_relaxed); }
}
