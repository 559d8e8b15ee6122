// wavenet_spec_kernels.hip -- the f16-split MFMA WaveNet block kernel as COMPILE-TIME layer chains for the official architectures.
//
// Reference arithmetic being replaced: WaveNetModelT / LayerArrayT / LayerT::Process, Conv1DT::Process, DenseLayerT::Process
// (NeuralAudio/WaveNet.h:768-799, 632-661, 462-494, 139-290, 336-383) with FastMath::Tanh (Activation.h:83-91).  The reference itself
// instantiates its templates once per official architecture (InternalModel.h:12-20, 152-159; WaveNet.h:503-661); so does this file.
//
// Same mapping, same operand images, same stream-state format and the same order of floating-point operations as the stage
// interpreter in wavenet_split_kernels.hip (so the two are interchangeable on a running stream and agree bit for bit), but nothing
// about the model is looked up at run time: the layer chain is unrolled, and dilation, ring offset and length, operand offsets in the
// weight image, image buffer parity, and the classification of every conv tap of every wave (all of its frames before the block:
// prefetched ring history only; all inside the block: LDS image only; straddling: both) are template constants.  What remains dynamic
// is per stream (ring cursors, state / row pointers).  Per layer and wave this removes the stage-descriptor load, ~80 scalar and ~40
// vector address instructions, the tap-classification branches and their basic blocks, the LDS round trip of the unshifted tap (the
// layer input's split quad stays in registers), the second aux read, the LDS publish when the next layer has no in-block tap
// (d >= block length), and the history loads / ring stores no wave of the block needs.
//
// Blocks must be exactly NF = 128, 64 or 32 frames (what audio hosts use); other sizes run on the interpreter -- same state, so a
// stream may alternate between the two.  Which launch runs which chain is decided in wavenet_choice.h (WaveNetLaunchFor); the launchers
// below are switches on that choice.
#include "wavenet_spec_impl.h"

namespace na
{
	// NA_WN_SPEC=0 (environment) or SetWaveNetSpecEnabled(false) (tests: both kernels on one stream in one process) turn the chains off
	static int& SpecSwitch()
	{
		// (NA_SP_T / NA_SP_GEN select interpreter variants: they imply it)
		static int on = Tuning::Get().wnSpecOff ? 0 : 1;
		return on;
	}
	bool WaveNetSpecEnabled() { return SpecSwitch() != 0; }
	void SetWaveNetSpecEnabled(bool on) { SpecSwitch() = on ? 1 : 0; }

	int WaveNetSpecArchId(const WnSplitStage* stages, int nstages, int stateF4, int wsplitQuads)
	{
		if (spk::Matches<spk::ArchStd>(stages, nstages, stateF4, wsplitQuads)) return WN_SPEC_STD;
		if (spk::Matches<spk::ArchLite>(stages, nstages, stateF4, wsplitQuads)) return WN_SPEC_LITE;
		if (spk::Matches<spk::ArchLite16>(stages, nstages, stateF4, wsplitQuads)) return WN_SPEC_LITE16;
		if (spk::Matches<spk::ArchA2Full>(stages, nstages, stateF4, wsplitQuads)) return WN_SPEC_A2FULL;
		if (spk::Matches<spk::ArchA2Lite>(stages, nstages, stateF4, wsplitQuads)) return WN_SPEC_A2LITE;
		return WN_SPEC_NONE;
	}

	// The chain of the family member the choice names (wavenet_choice.h ChainFor); the lite and A2 families live in their own translation units
	hipError_t LaunchWaveNetSpecFused(const WaveNetLaunchChoice& c, const WnFrameGroup* groups, int numGroups, const float* in, float* out, long inStride,
		long outStride, int n, hipStream_t stream)
	{
		if (c.kernel != WnLaunchKernel::Chain || c.nf != n) return hipErrorInvalidValue;
		switch (c.chain)
		{
		case WnChain::Std: return spk::LaunchChain<spk::FamStd, false>(c, groups, numGroups, in, out, inStride, outStride, stream);
		case WnChain::A2: return spk::LaunchSpecA2(c, groups, numGroups, in, out, inStride, outStride, stream);
		default: return spk::LaunchSpecLite(c, groups, numGroups, in, out, inStride, outStride, stream);
		}
	}

	// More groups than the kernarg segment holds, in one launch (wavenet_choice.h TableFor; wavenet_spec_impl.h WaveNetSpecTableKernel)
	hipError_t LaunchWaveNetSpecTable(const WaveNetLaunchChoice& c, const WnFrameGroup* groups, int numGroups, const float* in, float* out, long inStride,
		long outStride, int n, hipStream_t stream, WnLaunchTable& table)
	{
		if (c.kernel != WnLaunchKernel::ChainTable || c.nf != n) return hipErrorInvalidValue;
		switch (c.chain)
		{
		case WnChain::Std: return spk::LaunchChainTable<spk::FamStd, false>(c, groups, numGroups, in, out, inStride, outStride, stream, table);
		case WnChain::A2: return spk::LaunchSpecA2Table(c, groups, numGroups, in, out, inStride, outStride, stream, table);
		default: return spk::LaunchSpecLiteTable(c, groups, numGroups, in, out, inStride, outStride, stream, table);
		}
	}
}
