// wavenet_spec_lite_kernels.hip -- the specialised chains of the "lite" dilation lists (A1 Lite padded to 16 / 8 channels; two Feather or
// four Nano streams packed into one virtual stream): kernels of FamLite and FamLitePacked.  See wavenet_spec_kernels.hip.
#include "wavenet_spec_impl.h"

namespace na
{
	namespace spk
	{
		hipError_t LaunchSpecLite(const WaveNetLaunchChoice& c, const WnFrameGroup* groups, int numGroups, const float* in, float* out, long inStride, long outStride,
			hipStream_t stream)
		{
			switch (c.chain)
			{
			// (16 / 16 packed streams, at most one per CU: eight waves of one tile each, see ArchLite16T1)
			case WnChain::Lite16T1: return LaunchChain<FamLite16T1, true>(c, groups, numGroups, in, out, inStride, outStride, stream);
			case WnChain::LitePacked: return LaunchChain<FamLitePacked, true>(c, groups, numGroups, in, out, inStride, outStride, stream);
			case WnChain::Lite: return LaunchChain<FamLite, false>(c, groups, numGroups, in, out, inStride, outStride, stream);
			default: return hipErrorInvalidValue;
			}
		}

		// the same families as table launches (wavenet_launch.h LaunchWaveNetSpecTable)
		hipError_t LaunchSpecLiteTable(const WaveNetLaunchChoice& c, const WnFrameGroup* groups, int numGroups, const float* in, float* out, long inStride, long outStride,
			hipStream_t stream, WnLaunchTable& table)
		{
			switch (c.chain)
			{
			case WnChain::LitePacked: return LaunchChainTable<FamLitePacked, true>(c, groups, numGroups, in, out, inStride, outStride, stream, table);
			case WnChain::Lite: return LaunchChainTable<FamLite, false>(c, groups, numGroups, in, out, inStride, outStride, stream, table);
			default: return hipErrorInvalidValue;
			}
		}
	}
}
