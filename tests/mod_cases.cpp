// mod_cases.cpp -- drives csrc/mod_stage.h (ModStep, ModBook) with no device, for tests/test_mod_cpu.py: what the kernel and the batch
// do with the header, on the CPU -- the table, the rows' rings as the device keeps them, +0 in front of the line's start by position.
// Compiled with contraction off, like the step itself.  It also holds every sample against the two facts the kernel's shape rests on:
// a tap never reaches further back than the entry's `reach`, and with feedback no sample reads what its own chunk writes.
//
// usage: mod_cases [maxDelaySamples = 4096].  Commands on stdin, one per line; floats travel as the hexadecimal of their bits:
//   S row fadeSamples base depth phaseInc shape numVoices vp0 vp1 vp2 vp3 vg0 vg1 vg2 vg3 feedback wet dry tremoloDepth     a set call
//   R row fadeSamples                                                                 the modulation goes
//   L row                                                                             the stream is parked
//   X n, then ROWS lines of n samples                                                 a processing call of n samples
// Answers: after S / R / L "E <entries> <has modulation: per row> | <fade remaining: per row>" (refused calls print "! <text>");
// after X one line per entry, "Y row <n samples out>", then "E ...".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mod_stage.h"

using namespace na;

static constexpr int ROWS = 4;
static constexpr int kGroupWidth = 256; // the kernel's workgroup (mod_stage_kernels.hip)

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

// w[t - d] of sample j of the call, from the row's ring; +0 in front of the line's start, by position
struct RingLine
{
	const float* ring;
	unsigned mask, at;     // at: where the sample itself goes
	long long held;        // samples of the line in front of it
	int reach, chunkStart; // chunkStart: samples in front of the sample that belong to its chunk (feedback only), -1: none
	mutable bool broke = false;
	float operator()(int d) const
	{
		if (d < 1 || d > reach || (chunkStart >= 0 && d <= chunkStart)) broke = true;
		return (long long)d <= held ? ring[(at - (unsigned)d) & mask] : 0.0f;
	}
};

int main(int argc, char** argv)
{
	const int maxDelay = argc > 1 ? std::atoi(argv[1]) : kModMaxDelaySamples;
	if (maxDelay < kModMinDelaySamples || maxDelay > kModMaxDelaySamples) return 5;
	ModBook book;
	book.Configure(maxDelay);
	book.Resize(ROWS);
	const int ringSamples = book.RingSamples();
	// (the device never clears a ring: a pattern that would show in the bits stands where +0 has to come from positions)
	std::vector<float> rings((size_t)ROWS * ringSamples, 12345.678f);
	std::vector<ModEntry> table(ROWS);
	const auto entries = [&] {
		std::printf("E %d", book.NumEntries());
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.HasMod(s) ? 1 : 0);
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
			ModParams p;
			if (set)
			{
				std::string base, depth, fb, wet, dry, td, gain[kModMaxVoices];
				in >> base >> depth >> p.phaseInc >> p.shape >> p.numVoices;
				for (int v = 0; v < kModMaxVoices; v++) in >> p.voicePhase[v];
				for (int v = 0; v < kModMaxVoices; v++) in >> gain[v];
				in >> fb >> wet >> dry >> td;
				p.baseSamples = FromBits(base);
				p.depthSamples = FromBits(depth);
				for (int v = 0; v < kModMaxVoices; v++) p.voiceGain[v] = FromBits(gain[v]);
				p.feedback = FromBits(fb);
				p.wet = FromBits(wet);
				p.dry = FromBits(dry);
				p.tremoloDepth = FromBits(td);
				if (const char* why = ModParamsError(p, book.MaxDelay()))
				{
					std::printf("! %s\n", why);
					continue;
				}
			}
			// (the batch's rules: SetStreamMod refuses a set call during a fade, with the samples left, and a changed phase of a sounding voice)
			if (book.Fading(row))
			{
				std::printf("! fade %d\n", book.FadeRemaining(row));
				continue;
			}
			if (set && book.PhaseClash(row, p) >= 0)
			{
				std::printf("! phase %d\n", book.PhaseClash(row, p));
				continue;
			}
			book.Set(row, set ? &p : nullptr, N);
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
			if (count > ROWS) return 3;
			for (int c = 0; c < count; c++)
			{
				const ModEntry& e = table[c];
				if (e.reach < 3 || e.reach > maxDelay || e.chunk < 0) return 4;
				float* ring = rings.data() + (size_t)e.row * ringSamples;
				std::printf("Y %d", e.row);
				for (size_t i = 0; i < n; i++)
				{
					const long long k = (long long)e.k + (long long)i;
					float y = x[e.row][i];
					if (!(e.toNone && k >= e.N))
					{
						// the sample's place in its piece and, with feedback, in its chunk, as the kernel cuts them
						const int inPiece = (int)(i % (size_t)kModPieceSamples);
						const int chunk = e.chunk ? std::min(kGroupWidth, e.chunk) : 0;
						const RingLine at{ ring, (unsigned)ringSamples - 1u, e.pos + (unsigned)i, (long long)e.hist + (long long)i, e.reach, chunk ? inPiece % chunk : -1 };
						float w;
						y = ModStep(e, k, (unsigned long long)i, y, at, w);
						if (at.broke)
						{
							std::printf("\n! sample %zu of row %d reads outside its reach or inside its chunk\n", i, e.row);
							return 4;
						}
						ring[(e.pos + (unsigned)i) & ((unsigned)ringSamples - 1u)] = w;
					}
					std::printf(" %08x", Bits(y));
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
