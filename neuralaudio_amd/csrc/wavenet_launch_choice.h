// wavenet_launch_choice.h -- the launch half of THE decision of which kernel runs a WaveNet model (wavenet_choice.h has the other half and the
// overview): WaveNetLaunchFor, what ONE launch of one chunk decides from plain integers, and the knobs both halves read.  Kept apart
// because this half is all the kernel translation units need (through wavenet_launch.h): no plan, no model description.
// No HIP types, no environment and no Tuning::Get() inside the function: it works without a device (tests/test_wavenet_dispatch_cpu.py).
#pragma once

#include <algorithm>
#include <cstddef>

#include "frame_lds.h"
#include "tuning.h"
#include "wavenet_dev.h"

namespace na
{
	bool WaveNetSpecEnabled(); // wavenet_spec_kernels.hip: NA_WN_SPEC, flipped in a running process by NA_DebugSetWaveNetSpec

	constexpr int WN_FRAME_MAX_GROUPS = 8; // model groups in the kernarg segment of one launch

	// WaveNet kernel families: "split" = the f16-split MFMA kernels (wavenet_split_kernels.hip and the chains of wavenet_spec_kernels.hip),
	// "frame" = the f32 4x4x1-MFMA kernel (wavenet_frame_kernels.hip), "generic" = the runtime-shaped kernel for layer arrays wider than 16
	// channels (wavenet_generic_kernels.hip; frame-kernel state format).  A group stays in its family for life: the families keep
	// different stream-state formats.
	enum WnFamily { WN_FAMILY_AUTO, WN_FAMILY_SPLIT, WN_FAMILY_FRAME, WN_FAMILY_GENERIC };

	// the tuning knobs that take part in a choice (tuning.h: NA_WN_KERNEL, NA_WN_PACK, NA_WN_PAD, NA_WN_DENSE, NA_SP_T, NA_SP_SPB, NA_SP_GEN,
	// NA_SP_NO_T1, NA_FR_PF, NA_FR_SPB) and the chains' switch (NA_WN_SPEC)
	struct WaveNetKnobs
	{
		int wnKernel = 0, wnPack = -1;
		bool wnPadOff = false;
		int wnDense = -1;
		int spT = 0, spSpb = 0;
		bool spGen = false, spNoT1 = false;
		int frPrefetch = 1, frSpb = 0;
		bool specOn = true;
		// (specOn at call time: the switch is not a constant of the process)
		static WaveNetKnobs FromTuning()
		{
			const Tuning& t = Tuning::Get();
			return { t.wnKernel, t.wnPack, t.wnPadOff, t.wnDense, t.spT, t.spSpb, t.spGen, t.spNoT1, t.frPrefetch, t.frSpb, WaveNetSpecEnabled() };
		}
		// NA_WN_KERNEL=split|frame|generic forces one family for every model it can run (tuning / tests)
		WnFamily FamilyOverride() const { return wnKernel == 1 ? WN_FAMILY_SPLIT : (wnKernel == 2 ? WN_FAMILY_FRAME : (wnKernel == 3 ? WN_FAMILY_GENERIC : WN_FAMILY_AUTO)); }
	};

	inline bool WnSpecIsLite(int a) { return a == WN_SPEC_LITE || a == WN_SPEC_LITE16; }
	inline bool WnSpecIsA2(int a) { return a == WN_SPEC_A2FULL || a == WN_SPEC_A2LITE; }

	// ------------------------------------------------------------------------------------------ what one launch decides

	// one model group of a launch (wavenet_launch.h WnFrameGroup / WnModelDev), as plain integers
	struct WaveNetGroupFacts
	{
		int specArch;    // WnSpecArch
		int pack;        // > 1: packed group
		int splitFastT;  // WnModelDev::split_fast_T
		int numStreams;  // (virtual) streams
		int hasLists;    // the index lists are passed (slots != nullptr)
		int maxA4Floats; // frame kernel: largest staged block
		int maxG = 1, maxSplitOps = 16; // stage interpreter: what sizes its LDS (WnModelDev::max_G, max_split_ops)
	};
	struct WaveNetLaunchFacts
	{
		bool frame;      // the frame-kernel list (else a list of the f16-split kernels)
		int n;           // frames of the chunk
		const WaveNetGroupFacts* groups;
		int numGroups;
		int sharing;     // launches of this size that share the chip (free-running chains: 2)
		bool beyondCache; // the batch's stream state does not fit the Infinity Cache (wavenet_launch.h WnBeyondCacheBit)
		int cus;         // compute units of the device
	};

	enum class WnLaunchKernel
	{
		None,        // nothing is launched: `error` says why (0: nothing to do)
		Chain,       // WaveNetSpecKernel<family, NF, SPB, PK, NT>
		ChainTable,  // WaveNetSpecTableKernel<family, NF, SPB, PK>: more than WN_FRAME_MAX_GROUPS groups in one launch
		Interpreter, // WaveNetSplitKernel<T, SPB, WPS, GEN, PK>
		Frame,       // WaveNetFrameKernel<WPS, PF, SPB>
		Pieces,      // more than WN_FRAME_MAX_GROUPS groups and no table launch: the caller cuts the list into launches of eight and asks again
	};
	enum class WnChain { Std, Lite, LitePacked, Lite16T1, A2 }; // wavenet_spec_impl.h FamStd, FamLite, FamLitePacked, FamLite16T1, FamA2
	constexpr int WN_REFUSED_INVALID_VALUE = 1; // (hipErrorInvalidValue; wavenet_launch.h asserts the value)

	struct WaveNetLaunchChoice
	{
		WnLaunchKernel kernel = WnLaunchKernel::None;
		int error = 0;      // kernel == None: the hipError_t of the refusal
		int spb = 0;        // streams per workgroup (every kernel; the one-tile chain: in units of four-wave streams)
		WnChain chain = WnChain::Std; // chains ...
		int nf = 0;
		bool nt = false;    // ... with non-temporal ring traffic for the long dilations
		int t = 0, wps = 0; // interpreter: tiles per wave, waves per stream; frame kernel: wps
		bool gen = false;   // interpreter: the generic instantiation
		bool pk = false;    // chains / interpreter: the packed flavour
		int pf = 0;         // frame kernel: history prefetch (0 none, 1 registers, 2 LDS)
	};

	// dynamic LDS of WaveNetSplitKernel<T, spb, WPS, GEN, pk>: block images | planes | two weight buffers (wavenet_split_kernels.hip sp::Launch)
	constexpr size_t SPLIT_LDS_LIMIT = 160 * 1024;
	constexpr int SPLIT_PLANE_QUADS = 16 + WN_MAX_FRAMES; // wavenet_split_dev.h sp::PLANE
	constexpr size_t SplitLaunchLdsBytes(int spb, bool pk, int maxG, int maxOps)
	{
		return (pk ? (size_t)spb * 4 * WN_MAX_FRAMES * 8 : (size_t)spb * WN_MAX_FRAMES * 16) + (size_t)spb * 2 * maxG * SPLIT_PLANE_QUADS * 16 + (size_t)2 * maxOps * 64 * 16 + 1024;
	}

	namespace choice_detail
	{
		inline WaveNetLaunchChoice Refused(int error)
		{
			WaveNetLaunchChoice c;
			c.error = error;
			return c;
		}
		inline WaveNetLaunchChoice Chain(WnLaunchKernel kernel, WnChain chain, int nf, int spb, bool pk, bool nt = false)
		{
			WaveNetLaunchChoice c;
			c.kernel = kernel; c.chain = chain; c.nf = nf; c.spb = spb; c.pk = pk; c.nt = nt;
			return c;
		}

		// The table launch: more groups than the kernarg segment holds, ALL of one architecture family (all Standard; lite-family groups,
		// packed or not; the A2 submodels), blocks of 128 / 64 frames.  Streams per workgroup: two share the staged weights, so a group
		// with an odd stream count leaves half a workgroup idle -- with mostly one-stream groups (every stream its own model) the
		// half-size workgroups waste nothing.
		inline bool TableFor(const WaveNetLaunchFacts& f, const WaveNetKnobs& k, WaveNetLaunchChoice& out)
		{
			if ((f.n != 128 && f.n != 64) || !k.specOn || k.spSpb > 0) return false;
			const int arch = f.groups[0].specArch;
			const bool lite = WnSpecIsLite(arch), a2 = WnSpecIsA2(arch);
			if (arch != WN_SPEC_STD && !lite && !a2) return false;
			bool packed = false, lists = true, lite16 = false;
			long streams = 0, slots2 = 0;
			for (int i = 0; i < f.numGroups; i++)
			{
				const WaveNetGroupFacts& g = f.groups[i];
				const bool same = lite ? WnSpecIsLite(g.specArch) : (a2 ? WnSpecIsA2(g.specArch) : g.specArch == WN_SPEC_STD);
				if (g.numStreams <= 0 || !same) return false;
				packed = packed || g.pack > 1;
				lists = lists && g.hasLists != 0;
				lite16 = lite16 || g.specArch == WN_SPEC_LITE16;
				const int per2 = g.specArch == WN_SPEC_A2LITE ? 4 : 2; // streams per full-size workgroup of this architecture
				streams += g.numStreams;
				slots2 += (g.numStreams + per2 - 1) / per2 * per2;
			}
			// (only the lite family has a packed flavour, and it reads the index lists of every group; 16 / 16 only exists packed)
			if (packed ? (!lite || !lists) : lite16) return false;
			const int spb = (slots2 * 4 > streams * 5) ? 1 : 2; // more than a quarter of the full-size workgroups' stream slots would idle
			out = Chain(WnLaunchKernel::ChainTable, a2 ? WnChain::A2 : (lite ? (packed ? WnChain::LitePacked : WnChain::Lite) : WnChain::Std), f.n, spb, packed);
			return true;
		}

		// A specialised chain: every group the SAME official architecture family, blocks of exactly 128 / 64 / 32 frames (what audio
		// hosts use).  Same state as the interpreter, so a stream may alternate between the two.
		inline bool ChainFor(const WaveNetLaunchFacts& f, const WaveNetKnobs& k, WaveNetLaunchChoice& out)
		{
			if ((f.n != 128 && f.n != 64 && f.n != 32) || !k.specOn) return false;
			const int arch = f.groups[0].specArch;
			if (arch == WN_SPEC_NONE) return false;
			auto familyOf = [](int a) { return WnSpecIsLite(a) ? 1 : (WnSpecIsA2(a) ? 2 : 0); };
			const int fam = familyOf(arch);
			bool packed = false, lists = true, lite16 = false, all16 = true;
			int halfGroups = 0; // workgroups of the launch at SPB = 1 (an A2-Lite workgroup holds two streams there: T = 4)
			int virtualStreams = 0;
			for (int i = 0; i < f.numGroups; i++)
			{
				const WaveNetGroupFacts& g = f.groups[i];
				if (g.numStreams <= 0 || g.specArch == WN_SPEC_NONE || familyOf(g.specArch) != fam || (fam == 0 && g.specArch != arch)) return false;
				packed = packed || g.pack > 1;
				lists = lists && g.hasLists != 0;
				lite16 = lite16 || g.specArch == WN_SPEC_LITE16;
				all16 = all16 && g.specArch == WN_SPEC_LITE16;
				const int per = g.specArch == WN_SPEC_A2LITE ? 2 : 1;
				halfGroups += (g.numStreams + per - 1) / per;
				virtualStreams += g.numStreams;
			}
			// a packed launch reads the index lists of every group (a plain group riding along is pack = 1); only the lite family has one,
			// and 16 / 16 only exists packed
			if (packed ? (fam != 1 || !lists) : lite16) return false;
			// Streams per workgroup.  The half-size workgroups (SPB = 1: four waves) are compiled for two waves per SIMD, i.e. with 256 VGPRs
			// (spk::OccOf): a launch that cannot fill the chip anyway is bound by the latency of its few waves, and the registers let the
			// compiler keep a layer's LDS reads in flight (Nano x 1024 = 256 packed streams 25.1 -> 22.6 us, Feather x 1024 24.3 -> 22.2,
			// Standard x 512 25.4 -> 23.4).  They are used while every workgroup is resident at that occupancy: at most two per CU --
			// counting the workgroups of the launches that share the chip with this one (two free-running half-batch chains of 512 Standard
			// streams each: 37.1 us per step with the half-size workgroups, 36.7 with the full-size ones; Feather x 1024 = 2 x 256: 21.5 vs 24.8).
			const int wish = k.spSpb > 0 ? k.spSpb : (halfGroups * std::max(f.sharing, 1) > 2 * f.cus ? 2 : 1);
			const int spb = wish >= 2 ? 2 : 1;
			// a launch of 16 / 16 virtual streams only (packed Nano) with at most one of them per CU: one tile per wave, eight waves per stream
			// (Nano x 1024 = 256 virtual streams: a chain of 23 short stages, bound by what its few waves can issue); one stream per
			// workgroup (SPB = 2 in units of four-wave streams), every block length
			if (packed && all16 && !k.spNoT1 && k.spSpb == 0 && virtualStreams <= f.cus)
			{
				out = Chain(WnLaunchKernel::Chain, WnChain::Lite16T1, f.n, 2, true);
				return true;
			}
			// (a wave of a 4-tile architecture -- A2 Lite -- covers 64 frames)
			if (fam == 2 && f.n == 32) return false;
			const WnChain chain = fam == 0 ? WnChain::Std : (fam == 2 ? WnChain::A2 : (packed ? WnChain::LitePacked : WnChain::Lite));
			// (the non-temporal variant exists for full-size workgroups of 128-frame blocks: the regime it is for -- more state than the
			// Infinity Cache holds -- is thousands of streams)
			out = Chain(WnLaunchKernel::Chain, chain, f.n, spb, packed, f.beyondCache && f.n == 128 && spb == 2);
			return true;
		}

		// The stage interpreter takes everything else: runtime-shaped models, other block lengths, mixed launches.
		inline WaveNetLaunchChoice InterpreterFor(const WaveNetLaunchFacts& f, const WaveNetKnobs& k)
		{
			int total = 0, maxG = 1, maxOps = 16;
			// fast instantiation: every layer of every group has K == 3 and fills its lane mode (the official A1 architectures except Lite);
			// splitFastT = fewest tiles per wave it can run with (4 when an array has <= 4 channels), 0 = needs the generic one
			bool gen = k.spGen, packed = false, lists = true, allFast2 = true;
			int t = (k.spT == 2 || k.spT == 4) ? k.spT : 2;
			for (int i = 0; i < f.numGroups; i++)
			{
				const WaveNetGroupFacts& g = f.groups[i];
				if (g.numStreams <= 0) return Refused(WN_REFUSED_INVALID_VALUE);
				total += g.numStreams;
				if (g.splitFastT == 0) gen = true;
				else t = std::max(t, g.splitFastT);
				packed = packed || g.pack > 1;
				lists = lists && g.hasLists != 0;
				allFast2 = allFast2 && g.splitFastT == 2;
				maxG = std::max(maxG, g.maxG);
				maxOps = std::max(maxOps, g.maxSplitOps);
			}
			const int wish = k.spSpb > 0 ? k.spSpb : (total >= 512 ? 2 : 1);
			const int tiles = (f.n + 15) / 16;
			WaveNetLaunchChoice c;
			c.kernel = WnLaunchKernel::Interpreter;
			c.pk = packed;
			if (packed)
			{
				// packed groups (several real streams per virtual stream): the fast instantiation at 2 tiles per wave; plain groups may ride
				// along (pack = 1) if their plan is a fast one; the packed flavour always reads the index lists
				if (!allFast2 || !lists) return Refused(WN_REFUSED_INVALID_VALUE);
				c.t = 2;
				c.spb = wish >= 2 ? 2 : 1;
				c.wps = tiles > 4 ? 4 : (tiles > 2 ? 2 : 1);
			}
			else
			{
				c.gen = gen;
				c.t = t == 4 ? 4 : 2;
				c.wps = t == 4 ? (tiles > 4 ? 2 : 1) : (tiles > 4 ? 4 : (tiles > 2 ? 2 : 1));
				c.spb = (wish >= 4 && c.t == 2 && c.wps == 4) ? 4 : (wish >= 2 ? 2 : 1); // (four streams per workgroup: 128-frame blocks at 2 tiles per wave only)
			}
			if (SplitLaunchLdsBytes(c.spb, c.pk, maxG, maxOps) > SPLIT_LDS_LIMIT) return Refused(WN_REFUSED_INVALID_VALUE);
			return c;
		}

		inline WaveNetLaunchChoice FrameFor(const WaveNetLaunchFacts& f, const WaveNetKnobs& k)
		{
			int total = 0;
			int maxA4 = 0; // the launch's LDS follows the largest staged block among its groups
			for (int i = 0; i < f.numGroups; i++)
			{
				if (f.groups[i].numStreams <= 0) return Refused(WN_REFUSED_INVALID_VALUE);
				total += f.groups[i].numStreams;
				maxA4 = std::max(maxA4, f.groups[i].maxA4Floats);
			}
			// streams per workgroup: two streams share one staged copy of the weights once there are enough streams to cover all 256 CUs
			// (measured 1024 x Standard: SPB 1 / 2 / 4 = 61.5 / 61.3 / 65.0 us -- at 4 the 8-wave barrier skew eats the saving)
			const int wish = k.frSpb > 0 ? k.frSpb : (total >= 512 ? 2 : 1);
			WaveNetLaunchChoice c;
			c.kernel = WnLaunchKernel::Frame;
			c.wps = f.n > 64 ? 2 : 1;
			c.spb = 1;
			// ... the largest count up to that wish whose LDS fits (frame_lds.h): large kernels leave room for fewer block images beside
			// their staged weights, and the LDS history buffers of prefetch 2 give way to the register prefetch before a launch fails.
			// Precedence under NA_FR_PF=2: the knob asks for the LDS prefetch, so it is kept over the second stream -- <2,2,2>, then
			// <2,2,1>, and only where neither fits the register prefetch <2,1,2> / <2,1,1>.  One stream per workgroup with the register
			// prefetch fits every model that loaded (CheckWaveNetRunnable).  Blocks of at most 64 frames: one wave, no prefetch.
			if (f.n > 64 && k.frPrefetch != 0)
			{
				c.pf = 1;
				if (wish >= 4 && FrameLaunchFits(maxA4, 2, 4, 1)) c.spb = 4;
				else if (k.frPrefetch == 2 && wish >= 2 && FrameLaunchFits(maxA4, 2, 2, 2)) { c.pf = 2; c.spb = 2; }
				else if (k.frPrefetch == 2 && FrameLaunchFits(maxA4, 2, 1, 2)) c.pf = 2;
				else if (wish >= 2 && FrameLaunchFits(maxA4, 2, 2, 1)) c.spb = 2;
			}
			if (!FrameLaunchFits(maxA4, c.wps, c.spb, c.pf)) return Refused(WN_REFUSED_INVALID_VALUE);
			return c;
		}
	}

	inline WaveNetLaunchChoice WaveNetLaunchFor(const WaveNetLaunchFacts& f, const WaveNetKnobs& k)
	{
		using namespace choice_detail;
		if (f.n <= 0 || f.numGroups <= 0) return Refused(0);
		WaveNetLaunchChoice c;
		if (f.numGroups > WN_FRAME_MAX_GROUPS)
		{
			// a batch of many different models: ONE launch with the group table in device memory where the chains have one
			if (!f.frame && TableFor(f, k, c)) return c;
			c.kernel = WnLaunchKernel::Pieces;
			return c;
		}
		if (f.n > WN_MAX_FRAMES) return Refused(WN_REFUSED_INVALID_VALUE);
		if (f.frame) return FrameFor(f, k);
		if (ChainFor(f, k, c)) return c;
		return InterpreterFor(f, k);
	}
}
