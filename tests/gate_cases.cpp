// gate_cases.cpp -- drives csrc/gate_stage.h (GateStep, GateBegin, GateBook) with no device, for tests/test_gate_cpu.py: what the two
// kernels and the batch do with the header, on the CPU.  Compiled with contraction off, like the step itself.
//
// Commands on stdin, one per line; floats travel as the hexadecimal of their bits:
//   S row openPower closePower floorGain detectorCoeff attack hold release startOpen      a set call (refused constants print "! <text>")
//   R row                                                                              take the gate away
//   L row                                                                              the stream is parked
//   X n, then ROWS lines of n input samples                                            a processing call of n samples
// Answers: after S / R / L "E <entries> <has gate: per row>"; after X one line per entry "G row <n gains> | p hold open u", then "E ...".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gate_stage.h"

using namespace na;

static constexpr int ROWS = 4;

static float FromBits(const std::string& hex)
{
	const uint32_t b = (uint32_t)std::stoul(hex, nullptr, 16);
	float f;
	std::memcpy(&f, &b, 4);
	return f;
}
static uint32_t Bits(float f)
{
	uint32_t b;
	std::memcpy(&b, &f, 4);
	return b;
}

int main()
{
	GateBook book;
	book.Resize(ROWS);
	std::vector<GateState> state(ROWS);
	std::vector<GateEntry> table(ROWS);
	const auto entries = [&] {
		std::printf("E %d", book.NumEntries());
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.HasGate(s) ? 1 : 0);
		std::printf("\n");
	};
	std::string line;
	while (std::getline(std::cin, line))
	{
		std::istringstream in(line);
		std::string cmd;
		if (!(in >> cmd)) continue;
		if (cmd == "S")
		{
			int row, startOpen;
			std::string po, pc, fl, a;
			GateParams p;
			in >> row >> po >> pc >> fl >> a >> p.attackSamples >> p.holdSamples >> p.releaseSamples >> startOpen;
			p.openPower = FromBits(po);
			p.closePower = FromBits(pc);
			p.floorGain = FromBits(fl);
			p.detectorCoeff = FromBits(a);
			if (const char* why = GateParamsError(p))
			{
				std::printf("! %s\n", why);
				continue;
			}
			book.Set(row, p, startOpen != 0);
			entries();
		}
		else if (cmd == "R" || cmd == "L")
		{
			int row;
			in >> row;
			if (cmd == "R") book.Remove(row);
			else book.Leave(row);
			entries();
		}
		else if (cmd == "X")
		{
			size_t n;
			in >> n;
			std::vector<std::vector<float>> x(ROWS, std::vector<float>(n));
			for (int s = 0; s < ROWS; s++)
			{
				std::getline(std::cin, line);
				std::istringstream row(line);
				std::string hex;
				for (size_t i = 0; i < n; i++)
				{
					row >> hex;
					x[s][i] = FromBits(hex);
				}
			}
			const int count = book.BuildTable(table.data());
			for (int k = 0; k < count; k++)
			{
				const GateEntry& e = table[k];
				GateState s = GateBegin(e, state[e.row]);
				std::printf("G %d", e.row);
				for (size_t i = 0; i < n; i++) std::printf(" %08x", Bits(GateStep(e.c, e.forceOpen, s, x[e.row][i])));
				state[e.row] = s;
				std::printf(" | %08x %d %d %u\n", Bits(s.p), s.hold, s.open, s.u);
			}
			book.Advance(n);
			entries();
		}
		else return 2;
	}
	return 0;
}
