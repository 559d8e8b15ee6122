// launch_plan_cases.cpp -- tests/test_launch_plan_cpu.py: the launch plan (neuralaudio_amd/csrc/launch_plan.h) of each line of standard
// input, a sequence of group kinds by name.  One line out per line in: "<unit kind>:<group>,<group> ... | <halves> <resident>", the last
// two IsOneSplitLaunch with the packed launch / without it, at most 8 groups (WN_FRAME_MAX_GROUPS).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "launch_plan.h"

using na::LaunchKind;

static const char* const kNames[] = { "Frame", "Split", "SplitPacked", "Recurrent", "Own", "SplitJoinsPacked" };

int main()
{
	std::string line;
	while (std::getline(std::cin, line))
	{
		std::vector<LaunchKind> kinds;
		std::istringstream words(line);
		for (std::string w; words >> w;)
		{
			int k = 0;
			while (k < 6 && w != kNames[k]) k++;
			if (k == 6)
			{
				fprintf(stderr, "unknown kind %s\n", w.c_str());
				return 2;
			}
			kinds.push_back((LaunchKind)k);
		}
		const std::vector<na::LaunchUnit> units = na::PlanLaunches(kinds);
		for (const na::LaunchUnit& u : units)
		{
			printf("%s:", kNames[(int)u.kind]);
			for (size_t i = 0; i < u.groups.size(); i++) printf(i ? ",%d" : "%d", u.groups[i]);
			printf(" ");
		}
		printf("| %d %d\n", (int)na::IsOneSplitLaunch(units, true, 8), (int)na::IsOneSplitLaunch(units, false, 8));
	}
	return 0;
}
