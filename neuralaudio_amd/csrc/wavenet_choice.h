// wavenet_choice.h -- THE decision of which kernel runs a WaveNet model, in one place (the WaveNet counterpart of lstm_dev.h
// RecurrentKernelFor).  Two pure host functions of plain facts and of the tuning knobs that bear on them:
//   WaveNetKernelFor  what a model group decides ONCE, when it is created: kernel family, stream packing / padding, the specialised
//                     chain, the launch list its streams ride in -- and the plans it had to build to decide (gpu_groups.h WaveNetGroup
//                     keeps the answer; NA_BatchStreamKernelName, NA_ModelKernelInfo and NA_DebugWaveNetKernel report it);
//   WaveNetLaunchFor  what ONE launch of one chunk decides: exactly one kernel instantiation, or the error code of a launch that no
//                     kernel takes (the launchers -- wavenet_launch.h -- are switches on it; NA_DebugWaveNetLaunch asks it).
// No HIP types, no environment and no Tuning::Get() inside the functions: they work without a device (tests/test_wavenet_dispatch_cpu.py).
// DESIGN.md 6b has both decision tables.  The launch half and the knobs live in wavenet_launch_choice.h, which this header includes: the
// kernel translation units read that half alone.
#pragma once

#include <cmath>
#include <stdexcept>

#include "launch_plan.h"
#include "wavenet_launch_choice.h"
#include "wavenet_plan.h"

namespace na
{
	// which specialised chain (WnSpecArch) runs a split-kernel plan, WN_SPEC_NONE if none; host data (matched against the chains'
	// constexpr tables in wavenet_spec_kernels.hip)
	int WaveNetSpecArchId(const WnSplitStage* stages, int nstages, int stateF4, int wsplitQuads);

	// ------------------------------------------------------------------------------------------ what a group decides once

	struct WaveNetGroupChoice
	{
		WnFamily family = WN_FAMILY_FRAME;
		int pack = 1;            // real streams per virtual stream (1: no packing)
		bool dense = false;      // ... two streams per channel group in the last array
		bool isVirtual = false;  // packed and / or padded: `plan` describes the virtual model
		int specArch = WN_SPEC_NONE; // the specialised chain of `plan` (split family only)
		LaunchKind kind = LaunchKind::Frame;
		float inputLimit = INFINITY; // samples beyond +-limit are clamped by the kernel (f16-split arithmetic: split and generic families)
		bool rangeProven = true, weightsOk = true; // the range proof of the real model (wavenet_plan.cpp)
		WaveNetPlan plan;        // the plan the group runs, in its family's state format
		WaveNetPlan realPlan;    // isVirtual: the real model's plan (bookkeeping: bytes / MACs per REAL stream); empty otherwise

		// the kernel that runs the group's streams (rocprof name, without template arguments); a model with a specialised chain runs it for
		// blocks of 128 / 64 / 32 frames, the interpreter for other lengths
		const char* KernelName(bool specOn) const
		{
			if (family == WN_FAMILY_SPLIT) return (specArch != WN_SPEC_NONE && specOn) ? "WaveNetSpecKernel" : "WaveNetSplitKernel";
			return family == WN_FAMILY_GENERIC ? (plan.maxChannels > 64 ? "WaveNetWideKernel" : "WaveNetGenericKernel") : "WaveNetFrameKernel";
		}
		const char* FamilyName() const { return family == WN_FAMILY_SPLIT ? "f16-split" : (family == WN_FAMILY_GENERIC ? "generic" : "frame"); }
	};

	// the layout of a pack of `pack` streams (see "Dense packs" below; NA_DebugPackedWeights shows the weights of the same layout)
	inline bool WaveNetDenseFor(const WaveNetDesc& wn, int pack, const WaveNetKnobs& k) { return pack > 1 && k.wnDense != 0 && WaveNetPackCanBeDense(wn, pack); }

	// packHint: 0 = never pack (submodel of a container: its members go inactive), otherwise the number of streams the creating
	// AddStreams call brings.
	//
	// Family.  Measured on MI355X, 1024 streams x 128 frames: the f16-split kernel wins where its fast instantiation applies with 2 tiles
	// per wave (every array has 5..8 or 13..16 channels, K = 3: Standard 50 vs 60 us); narrow (Feather, Nano: <= 4-channel arrays) and
	// large-kernel (A2) models are faster on the frame kernel (33 / 30 / 71 us vs 44 / 44 / 133 us) -- but packed, padded, or on the A2
	// chains they are faster on the split kernels again (below).
	// May the f16-split kernels run a plan at all?  Their values are (hi, lo) pairs of f16: the plan builder proves statically that with
	// inputs inside +-condLimit (>= kSplitMinInputLimit) nothing leaves the f16 range and that the weights fit the operand format
	// (wavenet_plan.cpp).  A model that fails the proof runs on the f32 frame kernel -- no clamp, no overflow, the
	// reference's own number format -- and NA_BatchStreamKernelName says so; the proof outranks NA_WN_KERNEL=split.  One exception: the
	// official A2 shapes (LeakyReLU: the worst-case bound grows with the product of 23 layers' row sums and fails for every trained
	// model) stay on their chains, which saturate instead of overflowing and count the event (wavenet_split_dev.h SplitQuadSat,
	// NA_BatchStreamRangeEvents).
	// Packing (wavenet_plan.cpp PackWaveNetDesc): several streams of a NARROW model share one virtual stream of the f16-split kernel -- 4
	// streams for <= 4-channel arrays (Nano), 2 for <= 8 (Feather).  With the specialised chains it wins at every batch size (128-frame
	// blocks, us per step packed / f32 frame kernel: Nano 64 streams 19.5 / 24.5, 1024: 26.8 / 30.6, 4096: 61 / 113; Feather 64: 15.4 /
	// 26.5, 1024: 24.3 / 33.6), so every static narrow model that passes the proof runs packed, whatever the AddStreams call pattern --
	// the state layout of a group never depends on how its streams arrived (block-diagonal packing keeps every row sum, so the real
	// model's proof is the virtual model's).  NA_WN_PACK=0 turns packing off.
	// Dense packs (WaveNetPackCanBeDense: four Nano streams at 16 / 8 instead of 16 / 16 virtual channels -- half the ring traffic of the
	// second array, two tiles per MFMA in its thirteen layers): faster at every batch size (round 5, us per 128-frame step dense /
	// 16 x 16: 16 streams 15.3 / 16.0, 1024: 17.7 / 20.0, 4096: 32.4 / 48.2, 8192: 67.6 / 97.0).  NA_WN_DENSE=0: the 16 / 16 layout.
	// Padding without packing (WaveNetWantsPadding): a model whose arrays do not fill their lane mode (A1 Lite: 12 / 6 channels) is
	// widened to 16 / 8 and runs the fast flavour of the split kernel (1024 streams: 43.8 vs 46.0 us on the frame kernel, 1365: 66.4 vs
	// 76.0).  NA_WN_PAD=0 turns it off.
	inline WaveNetGroupChoice WaveNetKernelFor(const WaveNetDesc& wn, int packHint, const WaveNetKnobs& k)
	{
		WaveNetGroupChoice c;
		// the real model's plan in the f16-split state format: the family choice looks at its stage program and its range proof
		WaveNetPlan real = BuildWaveNetPlan(wn, true);
		c.rangeProven = real.splitRangeProven;
		c.weightsOk = real.splitWeightsOk;
		const int realSpec = real.genericOnly ? WN_SPEC_NONE : WaveNetSpecArchId(real.sstages.data(), (int)real.sstages.size(), real.stateF4, (int)(real.wsplit.size() / 8));
		const bool splitAllowed = !real.genericOnly && real.splitWeightsOk && real.rings.size() <= (size_t)WN_RANGE_EVENT_SLOT && (real.splitRangeProven || WnSpecIsA2(realSpec));
		const WnFamily o = k.FamilyOverride();
		const bool layoutFree = (o == WN_FAMILY_AUTO || o == WN_FAMILY_SPLIT) && splitAllowed; // packing / padding mean the split kernels
		if (layoutFree && packHint > 0 && k.wnPack != 0) c.pack = std::max(1, WaveNetPackFactor(wn));
		c.dense = WaveNetDenseFor(wn, c.pack, k);
		c.isVirtual = c.pack > 1 || (layoutFree && !k.wnPadOff && WaveNetWantsPadding(wn));
		if (c.isVirtual)
		{
			c.family = WN_FAMILY_SPLIT;
			c.plan = BuildPackedWaveNetPlan(wn, c.pack, c.dense);
			if (c.plan.splitFastT != 2) throw std::runtime_error("internal: packed / padded WaveNet plan is not a fast split-kernel plan");
			c.realPlan = std::move(real);
		}
		else
		{
			if (real.genericOnly) c.family = WN_FAMILY_GENERIC; // > 16 channels: the runtime-shaped kernel is the only one that runs it
			else if (o == WN_FAMILY_GENERIC) c.family = real.genericOk ? WN_FAMILY_GENERIC : WN_FAMILY_FRAME; // (conv heads: not in the runtime-shaped kernel)
			else if (o == WN_FAMILY_FRAME || !splitAllowed) c.family = WN_FAMILY_FRAME;
			// the A2 submodels have specialised chains on the split kernels' state format (round 3: 2048-stream quality sweep 120 us on the
			// frame kernel); their blocks that are not 128 / 64 frames fall to the stage interpreter
			else c.family = (o == WN_FAMILY_SPLIT || real.splitFastT == 2 || WnSpecIsA2(realSpec)) ? WN_FAMILY_SPLIT : WN_FAMILY_FRAME;
			// the two state formats size their rings differently (wavenet_plan.cpp AddRing): the other families get their own plan
			c.plan = c.family == WN_FAMILY_SPLIT ? std::move(real) : BuildWaveNetPlan(wn, false);
		}
		if (c.family == WN_FAMILY_SPLIT)
		{
			c.specArch = c.isVirtual ? WaveNetSpecArchId(c.plan.sstages.data(), (int)c.plan.sstages.size(), c.plan.stateF4, (int)(c.plan.wsplit.size() / 8)) : realSpec;
			c.kind = c.pack > 1 ? LaunchKind::SplitPacked : (c.plan.splitFastT == 2 ? LaunchKind::SplitJoinsPacked : LaunchKind::Split);
		}
		else c.kind = c.family == WN_FAMILY_GENERIC ? LaunchKind::Own : LaunchKind::Frame;
		if (c.family != WN_FAMILY_FRAME) c.inputLimit = c.plan.condLimit;
		return c;
	}
}
