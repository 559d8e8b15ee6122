// cabinet_stage_kernels.hip -- the device side of the cabinet stage (cabinet_stage.h): TWO launches per piece of a
// call behind the model launches, over a table of active entries only.  No reference counterpart (its hosts convolve on the CPU).
//
//   CabinetAppendKernel    copies the piece's raw samples from the row into the row's ring: the convolution works in place on the row
//                          and every output needs raw samples that another workgroup's outputs replace.
//   CabinetConvolveKernel  one workgroup per (entry, block of 128 outputs), 256 threads = 32 output quads x 8 tap slices.  The taps go
//                          through LDS in tiles of 1024 together with the window of the ring they meet (1024 + 128 samples, zeros in
//                          front of the stream's history); a thread owns four consecutive outputs and, in every tile, the 128 taps of
//                          its slice: per four taps one 128-bit LDS read of the taps (a broadcast), one of the next four window samples
//                          (the other four stay in registers), sixteen FMAs.  The eight partial sums of an output are added through
//                          LDS in rising slice number.  Tiles and slices beyond the IR's own length are skipped: the cost follows K.
//                          During a fade the block convolves a second time with the IR it fades from and blends the two.
//
// Order of one output's sum: cabinet_stage.h (CabSliceOf) -- a function of the tap index alone.  The window is addressed by absolute
// ring position, rows are read and written sample by sample: alignment, stride, the cut into calls and the number of entries never show.
// Rows without an entry are never touched.
#include <hip/hip_runtime.h>

#include "cabinet_stage.h"

namespace na
{
	namespace
	{
		constexpr int kCabThreads = 256;
		constexpr int kCabQuads = kCabBlockOutputs / 4;        // 32
		constexpr int kCabWindow = kCabTileTaps + kCabBlockOutputs; // window samples of a tile
		static_assert(kCabQuads * kCabSlices == kCabThreads, "a thread per (output quad, slice)");
		static_assert(kCabSliceTaps % 4 == 0 && kCabBlockOutputs % 4 == 0, "quads");

		unsigned long long gCabinetLaunches = 0;

		struct CabShared
		{
			alignas(16) float taps[kCabTileTaps];
			alignas(16) float window[kCabWindow];
			float partial[kCabSlices][kCabBlockOutputs];
		};

		// c_h of output `threadIdx.x` of the block (threads 0 .. 127; the others return 0): `b0` is the block's first sample in the piece,
		// `first` the ring index of the piece's first sample, `hist` the samples of history in front of it, `n` the piece's length
		__device__ __forceinline__ float CabConvolve(CabShared& sh, const float* __restrict__ taps, int K, const float* __restrict__ ring, unsigned mask,
			unsigned first, int hist, int b0, int n)
		{
			const int tid = (int)threadIdx.x;
			if (taps == nullptr)
			{
				// the dry path: y itself
				const int t = b0 + tid;
				return (tid < kCabBlockOutputs && t < n) ? ring[(first + (unsigned)t) & mask] : 0.0f;
			}
			const int q = tid & (kCabQuads - 1), s = tid / kCabQuads;
			float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
			for (int kt = 0; kt < K; kt += kCabTileTaps)
			{
				__syncthreads(); // (the previous tile, or the previous convolution's reduction, has been read)
				for (int j = tid; j < kCabTileTaps; j += kCabThreads) sh.taps[j] = (kt + j < K) ? taps[kt + j] : 0.0f;
				// window[j] = y[b0 - kt - kCabTileTaps + j] (piece-relative index `idx`): zero in front of the history and behind the piece
				for (int j = tid; j < kCabWindow; j += kCabThreads)
				{
					const int idx = b0 - kt - kCabTileTaps + j;
					sh.window[j] = (idx >= -hist && idx < n) ? ring[(first + (unsigned)idx) & mask] : 0.0f;
				}
				__syncthreads();
				const int k0 = s * kCabSliceTaps; // this thread's taps of the tile: k0 .. k0 + 127
				if (kt + k0 < K)
				{
					const int chunks = min(kCabSliceTaps, K - kt - k0 + 3) / 4;
					int m = kCabTileTaps + 4 * q - k0; // window index of y[t0 - k] for the quad's first output and the slice's first tap
					float4 hi = *reinterpret_cast<const float4*>(&sh.window[m]);
					for (int c = 0; c < chunks; c++, m -= 4)
					{
						const float4 h = *reinterpret_cast<const float4*>(&sh.taps[k0 + 4 * c]);
						const float4 lo = *reinterpret_cast<const float4*>(&sh.window[m - 4]);
						// v[4 + i - j] = y[t_i - k_j]; every output takes its taps in rising k
						const float v[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
						const float hh[4] = { h.x, h.y, h.z, h.w };
#pragma unroll
						for (int j = 0; j < 4; j++)
#pragma unroll
							for (int i = 0; i < 4; i++) acc[i] = fmaf(hh[j], v[4 + i - j], acc[i]);
						hi = lo;
					}
				}
			}
#pragma unroll
			for (int i = 0; i < 4; i++) sh.partial[s][4 * q + i] = acc[i];
			__syncthreads();
			float sum = 0.0f;
			if (tid < kCabBlockOutputs)
			{
				sum = sh.partial[0][tid];
#pragma unroll
				for (int p = 1; p < kCabSlices; p++) sum += sh.partial[p][tid];
			}
			return sum;
		}
	}

	__global__ __launch_bounds__(256) void CabinetAppendKernel(const CabLaunch L)
	{
		const CabEntry e = L.table[blockIdx.x];
		if (e.row < 0) return;
		const float* __restrict__ row = L.rows + (long long)e.row * L.stride + L.done;
		float* __restrict__ ring = L.rings + (long long)e.row * L.ringSamples;
		const unsigned mask = (unsigned)L.ringSamples - 1u;
		const unsigned first = e.pos + (unsigned)(L.done & mask);
		for (int i = (int)(blockIdx.y * blockDim.x + threadIdx.x); i < L.n; i += (int)(gridDim.y * blockDim.x)) ring[(first + (unsigned)i) & mask] = row[i];
	}

	__global__ __launch_bounds__(kCabThreads) void CabinetConvolveKernel(const CabLaunch L)
	{
		__shared__ CabShared sh;
		const CabEntry e = L.table[blockIdx.x];
		if (e.row < 0) return;
		float* __restrict__ row = L.rows + (long long)e.row * L.stride + L.done;
		const float* __restrict__ ring = L.rings + (long long)e.row * L.ringSamples;
		const unsigned mask = (unsigned)L.ringSamples - 1u;
		const unsigned first = e.pos + (unsigned)(L.done & mask);
		// (earlier pieces of the call are history too; never further back than the ring still holds once this piece is in it)
		const int hist = (int)min((unsigned long long)(L.ringSamples - L.n), (unsigned long long)e.hist + L.done);
		const int b0 = (int)blockIdx.y * kCabBlockOutputs;
		float out = CabConvolve(sh, e.tapsA, e.KA, ring, mask, first, hist, b0, L.n);
		if (e.fading)
		{
			const float from = CabConvolve(sh, e.tapsB, e.KB, ring, mask, first, hist, b0, L.n);
			const float w = OutStageWeightAt(e.N, (long long)e.fk + (long long)L.done + b0 + (int)threadIdx.x);
			out = (1.0f - w) * from + w * out;
		}
		const int t = b0 + (int)threadIdx.x;
		if (threadIdx.x < kCabBlockOutputs && t < L.n) row[t] = out;
	}

	unsigned long long CabinetStageLaunches() { return gCabinetLaunches; }

	hipError_t LaunchCabinetStage(const CabLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n <= 0) return hipSuccess;
		if (!L.table || !L.rows || !L.rings || L.n > kCabPieceSamples) return hipErrorInvalidValue;
		const unsigned blocks = (unsigned)((L.n + kCabBlockOutputs - 1) / kCabBlockOutputs);
		hipLaunchKernelGGL(CabinetAppendKernel, dim3((unsigned)L.count, (unsigned)((L.n + 255) / 256)), dim3(256), 0, stream, L);
		hipLaunchKernelGGL(CabinetConvolveKernel, dim3((unsigned)L.count, blocks), dim3(kCabThreads), 0, stream, L);
		gCabinetLaunches += 2;
		return hipGetLastError();
	}
}
