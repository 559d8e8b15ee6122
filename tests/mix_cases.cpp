// mix_cases.cpp -- csrc/mix_stage.h on its own, without a device (tests/test_mix_cpu.py): the host book driven through a scenario, the
// table entries it builds printed, and the step functions evaluated the way the kernel evaluates them -- every source of a sample
// first, then every output; the matrices from the set that travels with the table, filed into a block, or from the block.
//
// stdin, one command per line (floats as the hex of their bits):
//   resize ROWS
//   set M D R  s0 t0 .. s(M-1) t(M-1)  g[D*M]
//   clear S | leave S
//   call N   followed by ROWS lines of N floats (the rows) and ROWS lines of N floats (the input rows)
// stdout: for `call`, a line per entry "entry M D R k row[8] dryMask gainSet", "units U", then ROWS lines of N floats.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mix_stage.h"

using namespace na;

static float FromHex(const std::string& s)
{
	const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16);
	float f;
	std::memcpy(&f, &u, 4);
	return f;
}
static uint32_t Bits(float f)
{
	uint32_t u;
	std::memcpy(&u, &f, 4);
	return u;
}

int main()
{
	MixBook book;
	int rows = 0;
	std::vector<float> block; // [rows][kMixSetFloats]: what the device block holds
	std::vector<MixEntry> table;
	std::string line;
	while (std::getline(std::cin, line))
	{
		std::istringstream in(line);
		std::string cmd;
		if (!(in >> cmd)) continue;
		if (cmd == "resize")
		{
			in >> rows;
			book.Resize(rows);
			block.assign((size_t)rows * kMixSetFloats, 0.0f);
			table.assign((size_t)rows * kMixRowEntries, MixEntry());
		}
		else if (cmd == "set")
		{
			int M, D, R, ids[kMixMaxMembers], taps[kMixMaxMembers];
			float g[kMixMatrixFloats];
			in >> M >> D >> R;
			for (int j = 0; j < M; j++) in >> ids[j] >> taps[j];
			for (int c = 0; c < D * M; c++)
			{
				std::string h;
				in >> h;
				g[c] = FromHex(h);
			}
			book.Set(ids, taps, M, D, g, R);
		}
		else if (cmd == "clear" || cmd == "leave")
		{
			int s;
			in >> s;
			if (cmd == "leave") book.Leave(s);
			else if (book.GroupOf(s) >= 0) book.Clear(book.GroupOf(s));
		}
		else if (cmd == "call")
		{
			int n;
			in >> n;
			std::vector<float> y((size_t)rows * n), x((size_t)rows * n);
			for (std::vector<float>* a : { &y, &x })
				for (int r = 0; r < rows; r++)
				{
					std::getline(std::cin, line);
					std::istringstream v(line);
					for (int i = 0; i < n; i++)
					{
						std::string h;
						v >> h;
						(*a)[(size_t)r * n + i] = FromHex(h);
					}
				}
			int units = 0;
			const int count = book.BuildTable(table.data(), units);
			for (int e = 0; e < count; e++)
			{
				const MixEntry& m = table[(size_t)e];
				std::printf("entry %d %d %d %d", m.M, m.D, m.R, m.k);
				for (int j = 0; j < kMixMaxMembers; j++) std::printf(" %d", m.row[j]);
				std::printf(" %d %d\n", m.dryMask, m.gainSet);
				float* own = &block[(size_t)m.row[0] * kMixSetFloats];
				if (m.gainSet >= 0) std::memcpy(own, reinterpret_cast<const float*>(table.data() + count + m.gainSet * kMixSetEntries), sizeof(float) * kMixSetFloats);
				for (int i = 0; i < n; i++)
				{
					float src[kMixMaxMembers];
					for (int j = 0; j < m.M; j++) src[j] = (((m.dryMask >> j) & 1) ? x : y)[(size_t)m.row[j] * n + i];
					for (int d = 0; d < m.D; d++)
					{
						float acc = 0.0f;
						bool any = false;
						for (int j = 0; j < m.M; j++)
						{
							const int c = d * kMixMaxMembers + j;
							MixAccumulate(acc, any, MixGainAt(own[c], own[kMixMatrixFloats + c], m.R, (long long)m.k + i), src[j]);
						}
						y[(size_t)m.row[d] * n + i] = any ? acc : 0.0f;
					}
				}
			}
			std::printf("units %d\n", units);
			for (int r = 0; r < rows; r++)
			{
				for (int i = 0; i < n; i++) std::printf("%08" PRIx32 " ", Bits(y[(size_t)r * n + i]));
				std::printf("\n");
			}
			book.Advance((size_t)n);
		}
		else if (cmd == "state")
		{
			int s;
			in >> s;
			const int g = book.GroupOf(s);
			std::printf("state %d %d %d %d\n", g, book.NumGroups(), book.HasDry() ? 1 : 0, g >= 0 ? book.RampRemaining(g) : 0);
		}
	}
	return 0;
}
