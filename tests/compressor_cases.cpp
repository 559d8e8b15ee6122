// compressor_cases.cpp -- drives csrc/compressor_stage.h (CompLevel, CompFollow, CompCurveAt, CompGain, CompBook) with no device, for
// tests/test_compressor_cpu.py: what the kernel and the batch do with the header, on the CPU -- the table with the curves behind its
// entries, the rows' two curve slots and states as the device keeps them.  Compiled with contraction off, like the step itself.
//
// Commands on stdin, one per line; floats travel as the hexadecimal of their bits:
//   S row fadeSamples attackCoeff releaseCoeff, then one line of 513 curve values     a set call (refused ones print "! <text>")
//   R row fadeSamples                                                                 the compressor goes
//   L row                                                                             the stream is parked
//   X n, then ROWS lines of n samples                                                 a processing call of n samples
// Answers: after S / R / L "E <entries> <has compressor: per row> | <fade remaining: per row>"; after X two lines per entry,
// "G row <n gains> | e g" and "Y row <n samples out>", then "E ...".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "compressor_stage.h"

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
	CompBook book;
	book.Resize(ROWS);
	std::vector<CompState> state(ROWS);
	std::vector<CompCurve> curves(2 * ROWS); // [row][slot], as on the device
	std::vector<CompEntry> table((size_t)ROWS * kCompRowEntries);
	auto params = std::make_unique<CompParams>();
	const auto entries = [&] {
		std::printf("E %d", book.NumEntries());
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.HasCompressor(s) ? 1 : 0);
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
		if (cmd == "S" || cmd == "R")
		{
			int row, N;
			in >> row >> N;
			const bool set = cmd == "S";
			if (set)
			{
				std::string a, r, hex;
				in >> a >> r;
				params->attackCoeff = FromBits(a);
				params->releaseCoeff = FromBits(r);
				std::getline(std::cin, line);
				std::istringstream values(line);
				for (int i = 0; i < kCompCurvePoints; i++)
				{
					values >> hex;
					params->curve[i] = FromBits(hex);
				}
				const std::string why = CompParamsError(*params);
				if (!why.empty())
				{
					std::printf("! %s\n", why.c_str());
					continue;
				}
			}
			if (book.Fading(row))
			{
				std::printf("! fade %d\n", book.FadeRemaining(row)); // (the batch's rule: SetStreamCompressor refuses, with the samples left)
				continue;
			}
			book.Set(row, set ? params.get() : nullptr, N);
			entries();
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
					x[s][i] = FromBits(hex);
				}
			}
			int units = 0;
			const int count = book.BuildTable(table.data(), units);
			if (units > (int)table.size()) return 3;
			const CompCurve* travelled = reinterpret_cast<const CompCurve*>(table.data() + count);
			for (int k = 0; k < count; k++)
			{
				const CompEntry& e = table[k];
				// the curves that came with the table go into their slots, as the kernel files them
				if (e.coefTo >= 0) curves[(size_t)e.row * 2 + e.slotTo] = travelled[e.coefTo];
				if (e.coefFrom >= 0) curves[(size_t)e.row * 2 + (1 - e.slotTo)] = travelled[e.coefFrom];
				const float* tB = e.unityTo ? nullptr : curves[(size_t)e.row * 2 + e.slotTo].t;
				const float* tA = e.unityFrom ? nullptr : curves[(size_t)e.row * 2 + (1 - e.slotTo)].t;
				CompState s = state[e.row];
				if (e.start) s.e = 0.0f;
				std::vector<float> y(n);
				std::printf("G %d", e.row);
				for (size_t i = 0; i < n; i++)
				{
					s.e = CompFollow(e.aA, e.aR, s.e, CompLevel(x[e.row][i]));
					const float gB = tB ? CompCurveAt(tB, s.e) : 1.0f;
					float g = gB;
					if (e.fading)
					{
						const float w = OutStageWeightAt(e.N, (long long)e.fk + (long long)i);
						if (w != 1.0f) g = CompGain(w, tA ? CompCurveAt(tA, s.e) : 1.0f, gB);
					}
					s.g = g;
					y[i] = x[e.row][i] * g;
					std::printf(" %08x", Bits(g));
				}
				state[e.row] = s;
				std::printf(" | %08x %08x\nY %d", Bits(s.e), Bits(s.g), e.row);
				for (size_t i = 0; i < n; i++) std::printf(" %08x", Bits(y[i]));
				std::printf("\n");
			}
			book.Advance(n);
			entries();
		}
		else return 2;
	}
	return 0;
}
