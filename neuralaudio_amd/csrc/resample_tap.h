// resample_tap.h -- the per-output arithmetic both resamplers share (device code): the streaming stages of a resampling batch
// (resample_kernels.hip) and the whole-signal stages of NA_RenderOfflineAtRate (offline_resample_kernels.hip) include it, so that an
// output sample is the same f32 value on either path by construction: the same cleaning of an input sample, the same single FMA
// chain over the taps in the same order, the gain applied once behind the sum.
#pragma once

#include <hip/hip_runtime.h>

namespace na
{
	// NaN reads as silence, before the filter so that it cannot smear; infinities become the largest finite value
	__device__ __forceinline__ float ResampleCleanSample(float v) { return __builtin_isnan(v) ? 0.0f : fminf(fmaxf(v, -3.0e38f), 3.0e38f); }

	// ONE sum over the taps of a phase, newest sample first: c[t] meets win[idx - t].  Explicit fmaf: the chain does not depend on
	// what the compiler would contract.
	__device__ __forceinline__ float ResampleTapSum(const float* __restrict__ c, const float* win, int idx, int taps, float gain)
	{
		float acc = 0.0f;
		for (int t = 0; t < taps; t++) acc = fmaf(c[t], win[idx - t], acc);
		return acc * gain;
	}
}
