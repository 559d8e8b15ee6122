// frame_lds.h -- the dynamic LDS of one launch of the f32 frame kernel (wavenet_frame_kernels.hip), decided in ONE place: the launcher
// (fr::Launch), the choice of streams per workgroup (LaunchWaveNetFrameFused) and the load check (CheckWaveNetRunnable) all ask here, so a
// model that loads can run every buffer length at every stream count.  Host arithmetic only: no HIP header, so that it compiles and is
// tested on its own (tests/frame_lds_cases.cpp).
#pragma once

#include <algorithm>
#include <cstddef>

namespace na
{
	constexpr size_t FRAME_LDS_LIMIT = 160 * 1024; // what a workgroup of gfx950 can be granted
	constexpr int FRAME_HPF_LDS = 2;               // taps of ring history per wave in LDS (PF == 2)

	// float4 per thread staged per stage by the kernel's WeightStager: 6 KB per workgroup, rounded up to whole threads
	constexpr int FrameStagerWcopy(int nwaves) { return (384 + 64 * nwaves - 1) / (64 * nwaves); }

	// floats of a layer stage's staged block: K conv taps and the 1x1 (64 G floats each: one per lane and output group), then conv bias |
	// mix-in | 1x1 bias (4 G floats each)
	constexpr int FrameLayerBlockFloats(int ksize, int G) { return (ksize + 1) * 64 * G + 12 * G; }

	// float4 stride of the two LDS weight buffers: the largest staged block of the launch's groups, at least what the stager always writes
	constexpr int FrameWeightStrideF4(int maxA4Floats, int wps, int spb)
	{
		const int staged = FrameStagerWcopy(wps * spb) * 64 * wps * spb, block = (maxA4Floats + 3) / 4;
		return staged > block ? staged : block;
	}

	// bytes of dynamic LDS of WaveNetFrameKernel<wps, pf, spb>: block images [spb][2][4 groups][wps * 64 frames] float4
	// | weight buffers [2][stride] | pf == 2: history buffers [wps * spb waves][FRAME_HPF_LDS][4][64] float4.  maxA4Floats: the largest
	// staged block (floats) among ALL groups of the launch -- every workgroup gets the same allocation, whichever group it serves.
	constexpr size_t FrameLaunchLdsBytes(int maxA4Floats, int wps, int spb, int pf)
	{
		return (size_t)spb * 2 * wps * 4 * 64 * 16 + (size_t)2 * FrameWeightStrideF4(maxA4Floats, wps, spb) * 16 +
			(pf == 2 ? (size_t)wps * spb * FRAME_HPF_LDS * 4 * 64 * 16 : 0);
	}

	constexpr bool FrameLaunchFits(int maxA4Floats, int wps, int spb, int pf) { return FrameLaunchLdsBytes(maxA4Floats, wps, spb, pf) <= FRAME_LDS_LIMIT; }

	// What every model must fit to be loadable: one stream per workgroup, 128-frame blocks (two waves), history prefetch into registers
	// (or none: the same bytes).  More streams per workgroup and the LDS history buffers are taken only where they fit.
	constexpr bool FrameModelFits(int maxA4Floats) { return FrameLaunchFits(maxA4Floats, 2, 1, 1); }

	// the largest layer kernel size that loads at G channel groups
	inline int FrameMaxKernelSize(int G)
	{
		int k = 1;
		while (FrameModelFits(FrameLayerBlockFloats(k + 1, G))) k++;
		return k;
	}
}
