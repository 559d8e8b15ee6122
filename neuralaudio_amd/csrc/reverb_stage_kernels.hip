// reverb_stage_kernels.hip -- the device side of the reverb stage (reverb_stage.h): up to FOUR launches per piece of a
// call behind the cabinet stage, over a table of active entries only, and one launch per loaded IR on the load side.  No reference
// counterpart (its hosts convolve on the CPU).
//
//   ReverbAppendKernel    copies the piece's raw samples from the row into the row's ring: the stage works in place on the row, and
//                         the head of every output and the spectra need raw samples that another workgroup's outputs replace.
//   ReverbSpectrumKernel  one workgroup per (entry, block the piece completes): X_m = F([block m-1, block m]) from the ring into slot
//                         m mod slots of the row's ring of spectra.  Launched only where the piece completes a block of some entry.
//   ReverbTailKernel      one workgroup per (entry, block the piece needs a tail for, setting of a fade): a thread per bin walks j over
//                         the row's spectra and the IR's, 8 bytes of each per step, a wavefront reading 512 consecutive bytes; the sum
//                         goes through the inverse transform in LDS and the last 128 reals, scaled, are the block's tail, kept in the
//                         row's tail block of that setting for the calls that finish the block.  Launched only where a tail is needed.
//   ReverbApplyKernel     one workgroup per (entry, 128 outputs): the head's 128 taps direct form on the ring, head + tail, the mix
//                         and -- during a fade -- the second setting and the blend, written over the row.
//   ReverbIRKernel        load side: H_j of one partition of an IR.
//
// The transform is RevTransform below: 256 points in LDS, 128 butterflies a stage on threads 0 .. 127, the order reverb_stage.h
// states.  Every sample is addressed by its position since T0: alignment, stride, the cut into calls and the number of entries never
// show.  Rows without an entry are never touched.
#include <hip/hip_runtime.h>

#include "reverb_stage.h"

namespace na
{
	namespace
	{
		constexpr int kRevThreads = kRevPoints; // 256: a thread per bin
		constexpr int kRevApplyThreads = kRevPartition;
		constexpr unsigned kRevRingMask = (unsigned)kRevRingSamples - 1u;

		unsigned long long gReverbLaunches = 0;

		struct RevShared
		{
			float re[kRevPoints];
			float im[kRevPoints];
			float tw[kRevPoints];
		};

		__device__ __forceinline__ int RevBitReverse(int i) { return (int)(__brev((unsigned)i) >> 24); }

		// sh.re / sh.im hold u (the caller stored its value v[i] at index RevBitReverse(i)) and sh.tw the twiddles; on return they hold
		// F(v), or F'(v) with conj = -1.  All kRevThreads threads call it.
		__device__ __forceinline__ void RevTransform(RevShared& sh, float conj)
		{
			const int i = (int)threadIdx.x;
#pragma unroll
			for (int s = 1; s <= 8; s++)
			{
				__syncthreads();
				if (i < kRevPartition)
				{
					const int half = 1 << (s - 1);
					const int j = i & (half - 1);
					const int top = ((i - j) << 1) + j, bot = top + half;
					const int q = j << (8 - s);
					const RevComplex w = { sh.tw[2 * q], conj * sh.tw[2 * q + 1] };
					const RevComplex b = { sh.re[bot], sh.im[bot] };
					const RevComplex a = { sh.re[top], sh.im[top] };
					const RevComplex p = RevMul(w, b);
					const RevComplex lo = RevSub(a, p), hi = RevAdd(a, p);
					sh.re[bot] = lo.re;
					sh.im[bot] = lo.im;
					sh.re[top] = hi.re;
					sh.im[top] = hi.im;
				}
			}
			__syncthreads();
		}

		// the position of the piece's first sample and the blocks it touches
		struct RevPiece
		{
			long long t;  // since T0
			int o;        // t mod 128
			long long b0; // t / 128
		};
		__device__ __forceinline__ RevPiece RevPieceOf(const RevEntry& e, const RevLaunch& L)
		{
			RevPiece p;
			p.t = e.t + (long long)L.done;
			p.b0 = p.t / kRevPartition;
			p.o = (int)(p.t - p.b0 * kRevPartition);
			return p;
		}
	}

	__global__ __launch_bounds__(256) void ReverbAppendKernel(const RevLaunch L)
	{
		const RevEntry e = L.table[blockIdx.x];
		if (e.row < 0) return;
		const float* __restrict__ row = L.rows + (long long)e.row * L.stride + L.done;
		float* __restrict__ ring = L.rings + (long long)e.row * kRevRingSamples;
		const unsigned first = (unsigned)((unsigned long long)(e.t + (long long)L.done) & kRevRingMask);
		for (int i = (int)(blockIdx.y * blockDim.x + threadIdx.x); i < L.n; i += (int)(gridDim.y * blockDim.x)) ring[(first + (unsigned)i) & kRevRingMask] = row[i];
	}

	__global__ __launch_bounds__(kRevThreads) void ReverbSpectrumKernel(const RevLaunch L)
	{
		__shared__ RevShared sh;
		const RevEntry e = L.table[blockIdx.x];
		if (e.row < 0) return;
		const RevPiece p = RevPieceOf(e, L);
		if ((int)blockIdx.y >= (p.o + L.n) / kRevPartition) return; // (this entry completes fewer blocks)
		const long long m = p.b0 + (long long)blockIdx.y;
		const float* __restrict__ ring = L.rings + (long long)e.row * kRevRingSamples;
		const int i = (int)threadIdx.x;
		const long long at = (m - 1) * kRevPartition + i; // [block m-1, block m]
		const int r = RevBitReverse(i);
		sh.re[r] = at >= 0 ? ring[(unsigned)((unsigned long long)at & kRevRingMask)] : 0.0f;
		sh.im[r] = 0.0f;
		sh.tw[i] = L.twiddles[i];
		RevTransform(sh, 1.0f);
		float* __restrict__ X = L.spectra + ((long long)e.row * L.slots + (m % L.slots)) * kRevSpectrumFloats;
		*reinterpret_cast<float2*>(X + 2 * i) = make_float2(sh.re[i], sh.im[i]);
	}

	__global__ __launch_bounds__(kRevThreads) void ReverbTailKernel(const RevLaunch L)
	{
		__shared__ RevShared sh;
		const RevEntry e = L.table[blockIdx.x];
		if (e.row < 0) return;
		const RevSide side = blockIdx.z == 0 ? e.to : e.from;
		if (side.ir == nullptr) return; // (no second setting, or no reverb in it)
		const RevPiece p = RevPieceOf(e, L);
		const int touched = (p.o + L.n - 1) / kRevPartition + 1;
		// the first block the piece touches has its tail already when it began before the piece -- in an earlier piece of this call, or
		// in an earlier call if this setting was there
		const int skip = (p.o != 0 && (L.done > 0 || side.have)) ? 1 : 0;
		if ((int)blockIdx.y + skip >= touched) return;
		const long long b = p.b0 + skip + (long long)blockIdx.y;
		const int i = (int)threadIdx.x;
		sh.tw[i] = L.twiddles[i];
		const int J = (side.K + kRevPartition - 1) / kRevPartition;
		const int last = (int)min((long long)(J - 1), b);
		const float* __restrict__ H = side.ir + kRevPartition + 2 * i;
		const float* __restrict__ Xrow = L.spectra + (long long)e.row * L.slots * kRevSpectrumFloats + 2 * i;
		int slot = (int)((b - 1 + L.slots) % L.slots); // of X_{b-1}; (b = 0 has no term)
		RevComplex acc = { 0.0f, 0.0f };
#pragma unroll 4
		for (int j = 1; j <= last; j++)
		{
			const float2 h = *reinterpret_cast<const float2*>(H + (long long)(j - 1) * kRevSpectrumFloats);
			const float2 x = *reinterpret_cast<const float2*>(Xrow + (long long)slot * kRevSpectrumFloats);
			acc = RevAdd(acc, RevMul(RevComplex{ h.x, h.y }, RevComplex{ x.x, x.y }));
			slot = slot == 0 ? L.slots - 1 : slot - 1;
		}
		const int r = RevBitReverse(i);
		sh.re[r] = acc.re;
		sh.im[r] = acc.im;
		RevTransform(sh, -1.0f);
		if (i >= kRevPartition)
		{
			float* __restrict__ tail = L.tails + (((long long)e.row * 2 + side.tails) * kRevTailBlocks + (int)(b & (kRevTailBlocks - 1))) * kRevPartition;
			tail[i - kRevPartition] = sh.re[i] * 0.00390625f; // 2^-8
		}
	}

	namespace
	{
		struct RevApplyShared
		{
			float taps[2][kRevPartition];
			float window[2 * kRevPartition]; // window[j] = x[first - 128 + j]
		};

		// the output of one setting at position t (window index 128 + i): the row itself where the setting has no reverb
		__device__ __forceinline__ float RevSettingOutput(const RevApplyShared& sh, const RevSide& side, const float* taps, const float* __restrict__ tails, long long t, int i)
		{
			const float x = sh.window[kRevPartition + i];
			if (side.ir == nullptr) return x;
			const int K = min(side.K, kRevPartition);
			const int terms = (int)min((long long)K, t + 1); // k <= t
			float head = 0.0f;
			for (int k = 0; k < terms; k++) head = RevHeadStep(head, taps[k], sh.window[kRevPartition + i - k]);
			const long long b = t / kRevPartition;
			const float tail = tails[((long long)side.tails * kRevTailBlocks + (int)(b & (kRevTailBlocks - 1))) * kRevPartition + (int)(t - b * kRevPartition)];
			return RevMix(side.dry, side.wet, x, head, tail);
		}
	}

	__global__ __launch_bounds__(kRevApplyThreads) void ReverbApplyKernel(const RevLaunch L)
	{
		__shared__ RevApplyShared sh;
		const RevEntry e = L.table[blockIdx.x];
		if (e.row < 0) return;
		const RevPiece p = RevPieceOf(e, L);
		const int i = (int)threadIdx.x;
		const int first = (int)blockIdx.y * kRevApplyThreads; // of this workgroup's outputs, in the piece
		const float* __restrict__ ring = L.rings + (long long)e.row * kRevRingSamples;
		for (int j = i; j < 2 * kRevPartition; j += kRevApplyThreads)
		{
			const int idx = first - kRevPartition + j; // piece-relative
			const long long at = p.t + idx;
			sh.window[j] = (at >= 0 && idx < L.n) ? ring[(unsigned)((unsigned long long)at & kRevRingMask)] : 0.0f;
		}
		sh.taps[0][i] = (e.to.ir != nullptr && i < e.to.K) ? e.to.ir[i] : 0.0f;
		sh.taps[1][i] = (e.fading && e.from.ir != nullptr && i < e.from.K) ? e.from.ir[i] : 0.0f;
		__syncthreads();
		const int at = first + i;
		if (at >= L.n) return;
		const float* __restrict__ tails = L.tails + (long long)e.row * kRevTailFloats;
		const long long t = p.t + at;
		float out = RevSettingOutput(sh, e.to, sh.taps[0], tails, t, i);
		if (e.fading)
		{
			const float w = OutStageWeightAt(e.N, (long long)e.fk + (long long)L.done + at);
			if (w != 1.0f) out = RevBlend(w, RevSettingOutput(sh, e.from, sh.taps[1], tails, t, i), out);
		}
		L.rows[(long long)e.row * L.stride + (long long)L.done + at] = out;
	}

	__global__ __launch_bounds__(kRevThreads) void ReverbIRKernel(const RevIRLaunch L)
	{
		__shared__ RevShared sh;
		const int j = (int)blockIdx.x + 1;
		const int i = (int)threadIdx.x;
		const int r = RevBitReverse(i);
		sh.re[r] = i < kRevPartition ? L.taps[(long long)j * kRevPartition + i] : 0.0f;
		sh.im[r] = 0.0f;
		sh.tw[i] = L.twiddles[i];
		RevTransform(sh, 1.0f);
		*reinterpret_cast<float2*>(L.ir + kRevPartition + (long long)(j - 1) * kRevSpectrumFloats + 2 * i) = make_float2(sh.re[i], sh.im[i]);
	}

	unsigned long long ReverbStageLaunches() { return gReverbLaunches; }

	hipError_t LaunchReverbStage(const RevLaunch& L, hipStream_t stream)
	{
		if (L.count <= 0 || L.n <= 0) return hipSuccess;
		if (!L.table || !L.rows || !L.twiddles || !L.rings || !L.spectra || !L.tails || L.n > kRevPieceSamples || L.slots < kRevPieceBlocks
			|| L.spectrumBlocks < 0 || L.spectrumBlocks > kRevPieceBlocks || L.tailBlocks < 0 || L.tailBlocks > kRevPieceBlocks)
			return hipErrorInvalidValue;
		const unsigned blocks = (unsigned)((L.n + kRevApplyThreads - 1) / kRevApplyThreads);
		hipLaunchKernelGGL(ReverbAppendKernel, dim3((unsigned)L.count, (unsigned)((L.n + 255) / 256)), dim3(256), 0, stream, L);
		gReverbLaunches++;
		if (L.spectrumBlocks > 0)
		{
			hipLaunchKernelGGL(ReverbSpectrumKernel, dim3((unsigned)L.count, (unsigned)L.spectrumBlocks), dim3(kRevThreads), 0, stream, L);
			gReverbLaunches++;
		}
		if (L.tailBlocks > 0)
		{
			hipLaunchKernelGGL(ReverbTailKernel, dim3((unsigned)L.count, (unsigned)L.tailBlocks, 2), dim3(kRevThreads), 0, stream, L);
			gReverbLaunches++;
		}
		hipLaunchKernelGGL(ReverbApplyKernel, dim3((unsigned)L.count, blocks), dim3(kRevApplyThreads), 0, stream, L);
		gReverbLaunches++;
		return hipGetLastError();
	}

	hipError_t LaunchReverbIR(const RevIRLaunch& L, hipStream_t stream)
	{
		if (L.partitions <= 1) return hipSuccess;
		if (!L.taps || !L.ir || !L.twiddles) return hipErrorInvalidValue;
		hipLaunchKernelGGL(ReverbIRKernel, dim3((unsigned)(L.partitions - 1)), dim3(kRevThreads), 0, stream, L);
		return hipGetLastError();
	}
}
