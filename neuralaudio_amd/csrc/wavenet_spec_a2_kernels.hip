// wavenet_spec_a2_kernels.hip -- the specialised chains of the A2 slimmable model (NeuralModel.cpp:389-421: 23 layers of kernel size 6 / 15,
// conv head of 16 taps, LeakyReLU; 8 or 3 -> 4 channels): kernels of FamA2.  See wavenet_spec_kernels.hip.  (Compiled without
// -amdgpu-use-amdgpu-trackers: these long stages schedule better with the generic pressure trackers, 49.2 vs 50.3 us for A2 "Full".)
#include "wavenet_spec_impl.h"

namespace na
{
	namespace spk
	{
		hipError_t LaunchSpecA2(const WaveNetLaunchChoice& c, const WnFrameGroup* groups, int numGroups, const float* in, float* out, long inStride, long outStride,
			hipStream_t stream)
		{
			return LaunchChain<FamA2, false>(c, groups, numGroups, in, out, inStride, outStride, stream);
		}

		// ... as a table launch (wavenet_launch.h LaunchWaveNetSpecTable)
		hipError_t LaunchSpecA2Table(const WaveNetLaunchChoice& c, const WnFrameGroup* groups, int numGroups, const float* in, float* out, long inStride, long outStride,
			hipStream_t stream, WnLaunchTable& table)
		{
			return LaunchChainTable<FamA2, false>(c, groups, numGroups, in, out, inStride, outStride, stream, table);
		}
	}
}
