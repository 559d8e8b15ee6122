// eq_cases.cpp -- drives csrc/eq_stage.h (EqSectionStep, EqSanitize, EqMix, EqSectionsError, EqBook) with no device, for
// tests/test_eq_cpu.py: what the kernel and the batch do with the header -- the table, the two slots of a row, the coefficient sets that
// travel once -- on the CPU.  Compiled with contraction off, like the step itself.
//
// Commands on stdin, one per line; doubles and floats travel as the hexadecimal of their bits:
//   S row fade sections {b0 b1 b2 a1 a2} x sections      a set call (refused: "! <text>")
//   L row                                                the stream is parked
//   X n, then ROWS lines of n samples                    a processing call of n samples
// Answers: after S / L "E <entries> | <sections of the target: per row> | <fade remaining: per row>"; after X one line per entry
// "Y row <n outputs>", then "U <units uploaded> <coefficient sets among them>", "T row {x1 x2 y1 y2} x sections" per entry (the target
// cascade's states on the "device"), then "E ...".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eq_stage.h"

using namespace na;

static constexpr int ROWS = 4;

static float F32(const std::string& hex)
{
	const uint32_t b = (uint32_t)std::stoul(hex, nullptr, 16);
	float f;
	std::memcpy(&f, &b, 4);
	return f;
}
static double F64(const std::string& hex)
{
	const uint64_t b = (uint64_t)std::stoull(hex, nullptr, 16);
	double f;
	std::memcpy(&f, &b, 8);
	return f;
}
static uint32_t Bits(float f)
{
	uint32_t b;
	std::memcpy(&b, &f, 4);
	return b;
}
static unsigned long long Bits(double f)
{
	uint64_t b;
	std::memcpy(&b, &f, 8);
	return (unsigned long long)b;
}

int main()
{
	EqBook book;
	book.Resize(ROWS);
	std::vector<EqEntry> table((size_t)ROWS * kEqRowEntries);
	std::vector<EqCoefSet> coefs((size_t)ROWS * 2);                     // the device's blocks
	std::vector<EqSecState> state((size_t)ROWS * 2 * kEqMaxSections);
	const auto entries = [&] {
		std::printf("E %d |", book.NumEntries());
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.Target(s, nullptr, 0));
		std::printf(" |");
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.FadeRemaining(s));
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
			int row, fade, S;
			in >> row >> fade >> S;
			std::vector<EqSection> sec((size_t)std::max(S, 0));
			for (EqSection& c : sec)
			{
				std::string h[5];
				in >> h[0] >> h[1] >> h[2] >> h[3] >> h[4];
				c.b0 = F64(h[0]);
				c.b1 = F64(h[1]);
				c.b2 = F64(h[2]);
				c.a1 = F64(h[3]);
				c.a2 = F64(h[4]);
			}
			const std::string why = EqSectionsError(sec.data(), S);
			if (!why.empty()) std::printf("! %s\n", why.c_str());
			else if (fade < 0 || fade > kOutStageMaxRamp) std::printf("! fadeSamples must lie in [0, 1 << 20]\n");
			else if (book.Fading(row)) std::printf("! an EQ fade is running\n");
			else
			{
				book.Set(row, sec.data(), S, fade);
				entries();
			}
		}
		else if (cmd == "L")
		{
			int row;
			in >> row;
			book.Leave(row);
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
					x[s][i] = F32(hex);
				}
			}
			int units = 0;
			const int count = book.BuildTable(table.data(), units);
			const EqCoefSet* sets = reinterpret_cast<const EqCoefSet*>(table.data() + count);
			for (int q = 0; q < count; q++)
			{
				const EqEntry& e = table[(size_t)q];
				// what the kernel's lanes do at the start of a launch: coefficients filed, every state read before any is written
				const int slots[2] = { e.slotTo, 1 - e.slotTo };
				const int S[2] = { e.STo, e.fading ? e.SFrom : 0 };
				const int set[2] = { e.coefTo, e.fading ? e.coefFrom : -1 };
				const int src[2] = { e.srcTo, slots[1] };
				const int keep[2] = { e.keepTo, e.keepFrom };
				EqSecState st[2][kEqMaxSections];
				for (int h = 0; h < 2; h++)
					for (int i = 0; i < S[h]; i++)
					{
						if (set[h] >= 0) coefs[(size_t)e.row * 2 + slots[h]].s[i] = sets[set[h]].s[i];
						if (i < keep[h]) st[h][i] = state[((size_t)e.row * 2 + src[h]) * kEqMaxSections + i];
					}
				std::printf("Y %d", e.row);
				for (size_t t = 0; t < n; t++)
				{
					float o[2] = { 0.0f, 0.0f };
					for (int h = 0; h < (e.fading ? 2 : 1); h++)
					{
						double v = (double)EqSanitize(x[e.row][t]);
						for (int i = 0; i < S[h]; i++) v = EqSectionStep(coefs[(size_t)e.row * 2 + slots[h]].s[i], st[h][i], v);
						o[h] = (float)v;
					}
					std::printf(" %08x", Bits(e.fading ? EqMix(e.N, (long long)e.fk + (long long)t, o[1], o[0]) : o[0]));
				}
				std::printf("\n");
				for (int h = 0; h < 2; h++)
					for (int i = 0; i < S[h]; i++) state[((size_t)e.row * 2 + slots[h]) * kEqMaxSections + i] = st[h][i];
			}
			std::printf("U %d %d\n", units, (units - count) / kEqSetEntries);
			for (int q = 0; q < count; q++)
			{
				const EqEntry& e = table[(size_t)q];
				std::printf("T %d", e.row);
				for (int i = 0; i < e.STo; i++)
				{
					const EqSecState& s = state[((size_t)e.row * 2 + e.slotTo) * kEqMaxSections + i];
					std::printf(" %016llx %016llx %016llx %016llx", Bits(s.x1), Bits(s.x2), Bits(s.y1), Bits(s.y2));
				}
				std::printf("\n");
			}
			book.Advance(n);
			entries();
		}
		else return 2;
	}
	return 0;
}
