// delay_cases.cpp -- drives csrc/delay_stage.h (DelayStep, DelayBook) with no device, for tests/test_delay_cpu.py: what the kernel and
// the batch do with the header, on the CPU.  Compiled with contraction off, like the step itself.  The rings start full of a loud value
// and are never cleared: what lies in front of T0 must read as +0 by position.
//
// Commands on stdin, one per line; floats travel as the hexadecimal of their bits:
//   C maxDelaySamples                                       first line: the book's configuration
//   S row D feedback lowpassCoeff highpassCoeff wet dry N   a set call over N samples (refused: "! <text>")
//   N row fade                                              the set call with no parameters: no delay, over `fade` samples
//   L row                                                   the stream is parked
//   X n, then ROWS lines of n input samples                 a processing call of n samples
// Answers: after S / N / L "E <entries> <has delay: per row> | <fade remaining: per row>"; after X one line per entry
// "Y row <n outputs> | l q", then "E ...".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "delay_stage.h"

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
	DelayBook book;
	std::vector<std::vector<float>> rings;
	std::vector<DelayFilter> state(ROWS);
	std::vector<DelayEntry> table(ROWS);
	const auto entries = [&] {
		std::printf("E %d", book.NumEntries());
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.HasDelay(s) ? 1 : 0);
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
		if (cmd == "C")
		{
			int maxDelay;
			in >> maxDelay;
			book.Configure(maxDelay);
			book.Resize(ROWS);
			rings.assign(ROWS, std::vector<float>((size_t)book.RingSamples(), 12345.0f));
		}
		else if (cmd == "S" || cmd == "N")
		{
			int row, N;
			DelayParams p;
			if (cmd == "S")
			{
				std::string fb, aL, aH, wet, dry;
				in >> row >> p.delaySamples >> fb >> aL >> aH >> wet >> dry >> N;
				p.feedback = FromBits(fb);
				p.lowpassCoeff = FromBits(aL);
				p.highpassCoeff = FromBits(aH);
				p.wet = FromBits(wet);
				p.dry = FromBits(dry);
				if (const char* why = DelayParamsError(p, book.MaxDelay()))
				{
					std::printf("! %s\n", why);
					continue;
				}
			}
			else in >> row >> N;
			if (book.Fading(row))
			{
				std::printf("! a delay fade of stream %d is running\n", row);
				continue;
			}
			book.Set(row, cmd == "S" ? &p : nullptr, N);
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
			const int count = book.BuildTable(table.data());
			const unsigned mask = (unsigned)book.RingSamples() - 1u;
			for (int c = 0; c < count; c++)
			{
				const DelayEntry& e = table[c];
				std::vector<float>& ring = rings[e.row];
				DelayFilter s = e.start ? DelayFilter() : state[e.row];
				std::printf("Y %d", e.row);
				for (size_t i = 0; i < n; i++)
				{
					const long long k = (long long)e.k + (long long)i;
					float y = x[e.row][i];
					if (!(e.toNone && k >= e.N))
					{
						const long long held = (long long)e.hist + (long long)i;
						const unsigned p = e.pos + (unsigned)i;
						const float dB = held >= e.DB ? ring[(p - (unsigned)e.DB) & mask] : 0.0f;
						const float dA = held >= e.DA ? ring[(p - (unsigned)e.DA) & mask] : 0.0f;
						float w;
						y = DelayStep(e, s, OutStageWeightAt(e.N, k), y, dA, dB, w);
						ring[p & mask] = w;
					}
					std::printf(" %08x", Bits(y));
				}
				state[e.row] = s;
				std::printf(" | %08x %08x\n", Bits(s.l), Bits(s.q));
			}
			book.Advance(n);
			entries();
		}
		else return 2;
	}
	return 0;
}
