// drive_stage_kernels.hip -- the device side of the drive stage (drive_stage.h): per processing call with entries ONE
// launch, in front of the model launches, that fills the model-input block for every row of the batch -- a driven row oversampled,
// shaped and decimated, the others copied.  The caller's rows are only read.  No reference counterpart (its hosts run their pedals
// on the CPU).
//
// Work split: a workgroup is ONE wave and owns a row x a tile of 64 frames; the FIRs have no recurrence, so tiles are independent given
// their halo and a longer call is a wider grid (1024 rows x 128 frames: 2048 waves, two per SIMD).
//   1. the tile's 64 inputs and the 2 T = 64 behind them go to LDS (xs): from the caller's row, and behind the call's first sample from
//      the row's history block (zeros for a fresh entry) -- the only global reads of audio, one or two floats a lane.
//   2. up + shape: lanes run along the 64 + T base samples whose high-rate samples the tile reads; a lane computes the L phases of its
//      base sample, each one accumulator over T (+ 1) taps of xs, shapes them and stores them PHASE-MAJOR (ss[p][base]): 3 KB at L = 8.
//      The halo's s is recomputed, not stored: no high-rate history in memory, chunk-invariant by construction, T L shaper evaluations
//      more per tile (a third of the tile's own).
//   3. down: lane = output frame, one accumulator over the N + 1 taps in ascending j; tap j = L t + r reads phase (L - r) mod L at base
//      n - t - (r > 0), so the lanes of a wave read consecutive LDS words at every tap: conflict-free without padding.
// The coefficients are wave-uniform at every tap: they are read through uniform addresses of a read-only block, that is by scalar
// loads of 16 words into SGPRs, and the tap loops run in unrolled chunks of 16 FMAs with one LDS read each (fully unrolled the
// compiler loads every coefficient up front and spills 589 SGPRs).  `shape` is uniform for the
// workgroup: a scalar branch around the shaper, outside the tap loops.  The last tile of a call writes the row's next history block
// (the other one of the pair: the tiles of this call still read the first).
//
// Every sum is a chain of fmaf in the order of the contract; the unit is built without contraction, so nothing else fuses, and without
// compiler-made packed f32 (Makefile).
#include <hip/hip_runtime.h>

#include <atomic>

#include "drive_stage.h"

namespace na
{
	namespace
	{
		constexpr int kDriveTile = 64;                       // frames per wave
		constexpr int kDriveSpan = kDriveTile + kDriveTaps;  // base samples whose s a tile reads: n0 - T .. n0 + 63
		constexpr int kDriveWindow = kDriveTile + kDriveHistory;
		constexpr int kDriveChunk = 16;                      // coefficients per scalar load: the tap loops run in chunks of them
		std::atomic<unsigned long long> driveLaunches{ 0 };

		__device__ __forceinline__ float DriveClean(float v) { return v != v ? 0.0f : v; }

		// `shape` is uniform for the wave.  TANH: the StdMath form on the exp2 / rcp units, as the model kernels have it
		__device__ __forceinline__ float DriveShape(int shape, float v)
		{
			if (shape == kDriveShapeTanh) return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v * 2.885390081777927f) + 1.0f);
			if (shape == kDriveShapeCubic)
			{
				const float c = (v * v) * v, q = c / 3.0f, d = v - q;
				return fabsf(v) < 1.0f ? 1.5f * d : (v < 0.0f ? -1.0f : 1.0f);
			}
			return fminf(fmaxf(v, -1.0f), 1.0f);
		}

		template <int L>
		__device__ __forceinline__ void DriveTileOf(const DriveEntry& e, const float* __restrict__ coef, const float* xs, float* ss, int lane, long long first, unsigned long long n,
			float* __restrict__ out)
		{
			const float* __restrict__ down = coef;
			const float* __restrict__ up = coef + kDriveDownFloats;
			// up + shape: base sample b of the span is call sample first - T + b and xs[b + T]
			for (int b = lane; b < kDriveSpan; b += kDriveTile)
			{
				const long long k = e.done + first - kDriveTaps + b;
				const float g = DriveRampAt(e.from[0], e.to[0], e.R, k), bias = DriveRampAt(e.from[1], e.to[1], e.R, k);
				const float rest = DriveShape(e.shape, bias);
#pragma unroll
				for (int p = 0; p < L; p++)
				{
					float acc = 0.0f;
#pragma unroll 1
					for (int c = 0; c < kDriveTaps; c += kDriveChunk)
#pragma unroll
						for (int i = 0; i < kDriveChunk; i++) acc = fmaf(up[p * kDriveUpStride + c + i], xs[b + kDriveTaps - c - i], acc);
					if (p == 0) acc = fmaf(up[kDriveTaps], xs[b], acc);
					const float v = g * acc + bias;
					ss[p * kDriveSpan + b] = DriveShape(e.shape, v) - rest;
				}
			}
			__syncthreads();
			// down: frame `lane` of the tile is base sample lane + T of the span
			float acc = 0.0f;
#pragma unroll 1
			for (int c = 0; c < L * kDriveTaps; c += kDriveChunk)
			{
				const int t0 = c / L; // (L divides the chunk: tap c + i is t = t0 + i / L, r = i % L)
#pragma unroll
				for (int i = 0; i < kDriveChunk; i++)
				{
					const int r = i % L, t = t0 + i / L;
					acc = fmaf(down[c + i], r == 0 ? ss[lane + kDriveTaps - t] : ss[(L - r) * kDriveSpan + lane + kDriveTaps - t - 1], acc);
				}
			}
			acc = fmaf(down[L * kDriveTaps], ss[lane], acc);
			const long long k = e.done + first + lane;
			const float mix = DriveRampAt(e.from[2], e.to[2], e.R, k), level = DriveRampAt(e.from[3], e.to[3], e.R, k);
			const float wet = mix * acc, rem = 1.0f - mix, dry = rem * xs[lane + kDriveTaps], sum = wet + dry;
			if ((unsigned long long)(first + lane) < n) out[first + lane] = level * sum;
		}
	}

	__global__ __launch_bounds__(kDriveTile) void DriveStageKernel(const DriveEntry* __restrict__ table, int rows, const float* __restrict__ in, long inStride, float* __restrict__ out,
		long outStride, unsigned long long n, float* __restrict__ history, const float* __restrict__ coefs)
	{
		__shared__ float xs[kDriveWindow];                       // call samples first - 2 T .. first + 63
		__shared__ float ss[kDriveMaxOversample * kDriveSpan];   // [phase][base sample of the span]
		const int lane = threadIdx.x, row = blockIdx.y;
		const long long first = (long long)blockIdx.x * kDriveTile;
		if (row >= rows || (unsigned long long)first >= n) return;
		const DriveEntry e = table[row];
		const float* __restrict__ x = in + (long long)row * inStride;
		float* __restrict__ y = out + (long long)row * outStride;
		const bool known = e.oversample == 2 || e.oversample == 4 || e.oversample == 8;
		if (e.shape < 0 || e.shape > kDriveShapeHard || !known)
		{
			if ((unsigned long long)(first + lane) < n) y[first + lane] = x[first + lane];
			return;
		}
		const float* __restrict__ old = history + ((long long)row * 2 + (e.parity ? 1 : 0)) * kDriveHistory;
		for (int i = lane; i < kDriveWindow; i += kDriveTile)
		{
			const long long c = first - kDriveHistory + i;
			float v = 0.0f;
			if (c >= 0)
			{
				if ((unsigned long long)c < n) v = x[c];
			}
			else if (!e.fresh) v = old[kDriveHistory + c];
			xs[i] = DriveClean(v);
		}
		__syncthreads();
		const float* __restrict__ coef = coefs + DriveCoefSlot(e.oversample) * kDriveCoefFloats;
		if (e.oversample == 2) DriveTileOf<2>(e, coef, xs, ss, lane, first, n, y);
		else if (e.oversample == 4) DriveTileOf<4>(e, coef, xs, ss, lane, first, n, y);
		else DriveTileOf<8>(e, coef, xs, ss, lane, first, n, y);
		// the call's last tile: the 2 T samples behind the next call's first one, n - first of them from this tile's window on
		if ((unsigned long long)(first + kDriveTile) >= n)
		{
			float* __restrict__ next = history + ((long long)row * 2 + (e.parity ? 0 : 1)) * kDriveHistory;
			next[lane] = xs[(int)(n - (unsigned long long)first) + lane];
		}
	}

	hipError_t LaunchDriveStage(const DriveLaunch& L, hipStream_t stream)
	{
		if (L.rows <= 0 || L.n == 0) return hipSuccess;
		const unsigned long long tiles = (L.n + kDriveTile - 1) / kDriveTile;
		if (!L.table || !L.in || !L.out || !L.history || !L.coefs || L.rows > 65535 || tiles > 0x7FFFFFFFull || (long long)L.outStride < (long long)L.n) return hipErrorInvalidValue;
		hipLaunchKernelGGL(DriveStageKernel, dim3((unsigned)tiles, (unsigned)L.rows), dim3(kDriveTile), 0, stream, L.table, L.rows, L.in, L.inStride, L.out, L.outStride, L.n, L.history,
			L.coefs);
		driveLaunches.fetch_add(1, std::memory_order_relaxed);
		return hipGetLastError();
	}

	unsigned long long DriveStageLaunches() { return driveLaunches.load(std::memory_order_relaxed); }
}
