// meter_cases.cpp -- drives csrc/meter_stage.h (MeterSample, MeterMerge, MeterFold, MeterBook) with no device, for
// tests/test_meter_cpu.py: what the two kernels and the batch do with the header, on the CPU.  A call is walked the way the kernels walk
// it: cut at window boundaries (MeterRunLength), 64 lanes along the samples of a run, the lanes' partials merged pairwise, the run
// folded into the tap's state (MeterFold); the OUT tap leaves a record, and the book takes it in (Accept).
//
// Commands on stdin, one per line; floats travel as the hexadecimal of their bits:
//   S row window clipIn clipOut       a set call (refused constants print "! <text>")
//   R row                             take the meter away
//   L row                             the stream is parked
//   A row gen windows                 a record of generation `gen` with `windows` windows arrives for the row: prints "A <taken>"
//   X n, then ROWS lines of n input samples, ROWS lines of n output samples, ROWS lines of n gains or "-" (not gated)
// Answers: after S / R / L "E <entries> <has meter: per row> | <generation: per row>"; after X one line per entry
//   "M row has windows | energy oversTotal peak peakHold overs | (the same of the OUT tap) | gateGainMin gateGainLast windowSamples"
// (has: the book holds a reading of the row; the fields are those of that reading), then "E ...".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "meter_stage.h"

using namespace na;

static constexpr int ROWS = 4;
static constexpr int LANES = 64;

static float FromBits(const std::string& hex)
{
	const uint32_t b = (uint32_t)std::stoul(hex, nullptr, 16);
	float f;
	std::memcpy(&f, &b, 4);
	return f;
}

// one launch's work on one entry: the tap's state moves over n samples; true: a window was published into `pub`
static bool RunTap(const MeterEntry& e, bool out, MeterTapState& s, const float* x, const float* g, size_t n, MeterTapReading& pub, uint32_t& gateMin, uint32_t& pubMin, uint32_t& pubLast)
{
	bool published = false;
	const uint32_t W = (uint32_t)e.window, clip = out ? e.clipOutBits : e.clipInBits;
	for (size_t i = 0; i < n;)
	{
		const uint32_t len = MeterRunLength(s.pos, W, n - i);
		MeterPartial lanes[LANES];
		uint32_t gmin[LANES];
		for (int l = 0; l < LANES; l++)
		{
			gmin[l] = kMeterNoGainBits;
			for (uint32_t j = (uint32_t)l; j < len; j += LANES)
			{
				MeterSample(lanes[l], x[i + j], clip);
				if (out) gmin[l] = std::min(gmin[l], g ? MeterBits(g[i + j]) : kMeterOneBits);
			}
		}
		for (int step = 1; step < LANES; step *= 2)
			for (int l = 0; l < LANES; l += 2 * step)
			{
				MeterMerge(lanes[l], lanes[l + step]);
				gmin[l] = std::min(gmin[l], gmin[l + step]);
			}
		if (out) gateMin = std::min(gateMin, gmin[0]);
		if (MeterFold(s, lanes[0], len, W, pub))
		{
			published = true;
			if (out)
			{
				pubMin = gateMin;
				pubLast = g ? MeterBits(g[i + len - 1]) : kMeterOneBits;
				gateMin = kMeterNoGainBits;
			}
		}
		i += len;
	}
	return published;
}

static void PrintTap(const MeterTapReading& t)
{
	std::printf(" | %llu %llu %08x %08x %u", t.energy, t.oversTotal, MeterBits(t.peak), MeterBits(t.peakHold), t.overs);
}

int main()
{
	MeterBook book;
	book.Resize(ROWS);
	std::vector<MeterState> state(ROWS);
	std::vector<MeterEntry> table(ROWS);
	const auto entries = [&] {
		std::printf("E %d", book.NumEntries());
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.HasMeter(s) ? 1 : 0);
		std::printf(" |");
		for (int s = 0; s < ROWS; s++) std::printf(" %u", book.Gen(s));
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
			int row;
			std::string ci, co;
			MeterParams p;
			in >> row >> p.windowSamples >> ci >> co;
			p.clipLevelIn = FromBits(ci);
			p.clipLevelOut = FromBits(co);
			if (const char* why = MeterParamsError(p))
			{
				std::printf("! %s\n", why);
				continue;
			}
			book.Set(row, p);
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
		else if (cmd == "A")
		{
			MeterRecord rec;
			in >> rec.row >> rec.gen >> rec.reading.windows;
			std::printf("A %d\n", book.Accept(rec) ? 1 : 0);
		}
		else if (cmd == "X")
		{
			size_t n;
			in >> n;
			std::vector<std::vector<float>> rows[3];
			std::vector<char> gated(ROWS, 0);
			for (int what = 0; what < 3; what++)
			{
				rows[what].assign(ROWS, std::vector<float>(n));
				for (int s = 0; s < ROWS; s++)
				{
					std::getline(std::cin, line);
					std::istringstream row(line);
					std::string hex;
					if (what == 2 && line.rfind("-", 0) == 0) continue;
					if (what == 2) gated[s] = 1;
					for (size_t i = 0; i < n; i++)
					{
						row >> hex;
						rows[what][s][i] = FromBits(hex);
					}
				}
			}
			const int count = book.BuildTable(table.data());
			std::vector<MeterRecord> records((size_t)count);
			for (int k = 0; k < count; k++)
			{
				MeterEntry& e = table[k];
				e.gated = gated[e.row];
				MeterState& st = state[e.row];
				MeterTapReading pub;
				uint32_t unused = kMeterNoGainBits, a = 0, b = 0;
				// the IN launch
				MeterTapState s = MeterBegin(e, st.in);
				if (RunTap(e, false, s, rows[0][e.row].data(), nullptr, n, pub, unused, a, b)) st.latest.in = pub;
				st.in = s;
				// the OUT launch
				s = MeterBegin(e, st.out);
				uint32_t gateMin = e.start == kMeterStartFresh ? kMeterNoGainBits : st.gateMinBits, pubMin = kMeterOneBits, pubLast = kMeterOneBits;
				if (RunTap(e, true, s, rows[1][e.row].data(), e.gated ? rows[2][e.row].data() : nullptr, n, pub, gateMin, pubMin, pubLast))
				{
					st.latest.out = pub;
					st.latest.gateGainMin = MeterFloat(pubMin);
					st.latest.gateGainLast = MeterFloat(pubLast);
				}
				st.out = s;
				st.gateMinBits = gateMin;
				st.gen = e.gen;
				st.latest.windows = s.windows;
				st.latest.windowSamples = e.window;
				records[(size_t)k].row = e.row;
				records[(size_t)k].gen = e.gen;
				records[(size_t)k].reading = st.latest;
			}
			book.Advance(n);
			for (const MeterRecord& rec : records) (void)book.Accept(rec);
			for (int k = 0; k < count; k++)
			{
				const int row = table[k].row;
				const MeterReading r = book.HasReading(row) ? book.Latest(row) : MeterReading();
				std::printf("M %d %d %llu", row, book.HasReading(row) ? 1 : 0, r.windows);
				PrintTap(r.in);
				PrintTap(r.out);
				std::printf(" | %08x %08x %d\n", MeterBits(r.gateGainMin), MeterBits(r.gateGainLast), r.windowSamples);
			}
			entries();
		}
		else return 2;
	}
	return 0;
}
