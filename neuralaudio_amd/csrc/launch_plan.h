// launch_plan.h -- which model groups of a batch share a launch (GpuBatch::ProcessDevice and everything that asks how many launches a
// buffer takes).  Host data only: no HIP header, so that the rule compiles and is tested on its own (tests/test_launch_plan_cpu.py).
#pragma once

#include <algorithm>
#include <vector>

namespace na
{
	// How a model group's streams get onto the chip -- fixed for the life of the group (family, pack and plan are, and the tuning knobs
	// are read once per process).  The first five are also the kinds of launch units, in the order a buffer issues them.
	enum class LaunchKind
	{
		Frame,            // WaveNet frame kernel: the fused frame-kernel launch
		Split,            // f16-split kernel: the fused split launch
		SplitPacked,      // f16-split kernel with packed streams: the fused packed launch
		Recurrent,        // LSTM / GRU with an LDS-free kernel instance: the fused RecurrentDppKernel launch
		Own,              // a launch of its own (runtime-shaped WaveNet kernel, recurrent kernels that need LDS)
		SplitJoinsPacked, // f16-split kernel whose plan runs the fast flavour: the packed launch when the batch has one, else the split launch
	};

	struct LaunchUnit
	{
		LaunchKind kind;         // Frame | Split | SplitPacked | Recurrent | Own
		std::vector<int> groups; // indices into the planner's input; the first group owns the unit (lends it its side stream and done event)
	};

	// The launch units of a buffer, given the kinds of the groups that have active streams, in group order.  Groups that can share a
	// launch are fused: the WaveNet groups of one kernel family into one launch (frame kernel | f16-split kernel | f16-split kernel with
	// packed streams), all LSTM / GRU groups with an LDS-free kernel instance into another -- the workgroups of all architectures share
	// the chip, no fork / join per group.  Everything else runs on its own.  A plain split group whose plan runs the fast flavour rides
	// in the packed launch when there is one (then it passes its index lists even when its streams are contiguous), behind the packed
	// groups; without one it joins the plain split launch, behind that list's own groups.  Units come in the order frame list, split
	// list, packed list, recurrent list, then each group of its own in group order; the units are independent (disjoint rows, disjoint
	// state), and one unit runs directly on the batch stream.
	inline std::vector<LaunchUnit> PlanLaunches(const std::vector<LaunchKind>& kinds)
	{
		const bool packed = std::find(kinds.begin(), kinds.end(), LaunchKind::SplitPacked) != kinds.end();
		const LaunchKind joined = packed ? LaunchKind::SplitPacked : LaunchKind::Split;
		std::vector<LaunchUnit> units;
		for (LaunchKind list : { LaunchKind::Frame, LaunchKind::Split, LaunchKind::SplitPacked, LaunchKind::Recurrent })
		{
			LaunchUnit u = { list, {} };
			for (size_t i = 0; i < kinds.size(); i++)
				if (kinds[i] == list) u.groups.push_back((int)i);
			for (size_t i = 0; i < kinds.size() && list == joined; i++)
				if (kinds[i] == LaunchKind::SplitJoinsPacked) u.groups.push_back((int)i);
			if (!u.groups.empty()) units.push_back(std::move(u));
		}
		for (size_t i = 0; i < kinds.size(); i++)
			if (kinds[i] == LaunchKind::Own) units.push_back({ LaunchKind::Own, { (int)i } });
		return units;
	}

	// The buffer is ONE launch of the f16-split kernels -- the plain split launch, or with `packedToo` the packed one -- of at most
	// `maxGroups` groups: what the half-batch chains (plain or packed) and the resident launch (plain only) can take over.
	inline bool IsOneSplitLaunch(const std::vector<LaunchUnit>& units, bool packedToo, size_t maxGroups)
	{
		return units.size() == 1 && (units[0].kind == LaunchKind::Split || (packedToo && units[0].kind == LaunchKind::SplitPacked)) &&
			units[0].groups.size() <= maxGroups;
	}
}
