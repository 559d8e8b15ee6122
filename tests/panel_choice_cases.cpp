// panel_choice_cases.cpp -- WaveNetExactF32LaunchFor (csrc/wavenet_launch_choice.h) for tests/test_panel_f32_cpu.py: one line
// "wideNb panelNb maxFrames" per (maxChannels, gated) pair on the command line.
#include <cstdio>
#include <cstdlib>

#include "wavenet_launch_choice.h"

int main(int argc, char** argv)
{
	for (int i = 1; i + 1 < argc; i += 2)
	{
		const na::WaveNetExactF32LaunchChoice c = na::WaveNetExactF32LaunchFor(atoi(argv[i]), atoi(argv[i + 1]) != 0);
		printf("%d %d %d\n", c.wideNb, c.panelNb, c.maxFrames);
	}
	return 0;
}
