// frame_lds_cases.cpp -- tests/test_host_cpu.py: the LDS arithmetic of the f32 frame kernel's launches (neuralaudio_amd/csrc/frame_lds.h)
// for each line of standard input "<channels> <kernel size> <waves per stream> <streams per workgroup> <prefetch>".  One line out per
// line in: "<block floats> <stride float4> <LDS bytes> <fits> <model fits> <largest kernel size at this width>".
#include <cstdio>

#include "frame_lds.h"

int main()
{
	int channels, ksize, wps, spb, pf;
	while (scanf("%d %d %d %d %d", &channels, &ksize, &wps, &spb, &pf) == 5)
	{
		const int G = (channels + 3) / 4, block = na::FrameLayerBlockFloats(ksize, G);
		printf("%d %d %zu %d %d %d\n", block, na::FrameWeightStrideF4(block, wps, spb), na::FrameLaunchLdsBytes(block, wps, spb, pf),
			(int)na::FrameLaunchFits(block, wps, spb, pf), (int)na::FrameModelFits(block), na::FrameMaxKernelSize(G));
	}
	return 0;
}
