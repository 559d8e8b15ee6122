// tuner_cases.cpp -- drives csrc/tuner_stage.h (TunerQuantise, TunerGroupSum, TunerLagSum, the selection's tests, TunerBook) with no
// device, for tests/test_tuner_cpu.py: what the two kernels and the batch do with the header, on the CPU.  A call is walked the way
// the kernels walk it: in pieces of kTunerPieceSamples; 64 lanes along the decimated samples of a piece, lane 0 joining the carried
// part of the open group and leaving the next one (the append launch); then, for the entries whose last evaluation end lies in the
// piece, the span out of the ring, 256 threads along the lags, a min of t, a max of r, a min of t, and e[] at the three lags the
// reading holds (the evaluate launch); the records go into the book (Accept).
//
// Commands on stdin, one per line; floats travel as the hexadecimal of their bits:
//   S row decimation windowSamples minLag maxLag hopSamples phase thresholdQ10 minEnergy     a set call (refused constants print "! <text>")
//   R row                             take the tuner away
//   L row                             the stream is parked
//   A row gen evaluations             a record of generation `gen` with `evaluations` arrives for the row: prints "A <taken>"
//   X n, then ROWS lines of n input samples
// Answers: after S / R / L "E <entries> <has tuner: per row> | <generation: per row>"; after X one line per entry
//   "T row has evaluations position lag decimation e0 r r r e e e"
// (has: the book holds a reading of the row; the fields are those of that reading), then "E ..." with " | <evaluating entries>" behind it.
#include <climits>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tuner_stage.h"

using namespace na;

static constexpr int ROWS = 4;
static constexpr int LANES = 64, THREADS = 256;
static constexpr int MASK = kTunerRingSamples - 1;

static float FromBits(const std::string& hex)
{
	const uint32_t b = (uint32_t)std::stoul(hex, nullptr, 16);
	float f;
	std::memcpy(&f, &b, 4);
	return f;
}

// TunerAppendKernel on one entry: samples [offset, offset + n) of the call
static void Append(const TunerEntry& e, const float* row, unsigned long long offset, unsigned long long n, TunerState& st, int* ring)
{
	const int D = e.decimation;
	const float* x = row + offset;
	const unsigned long long first = e.pos + offset, end = first + n;
	const long long mFirst = (long long)(first / (unsigned long long)D), mEnd = (long long)(end / (unsigned long long)D);
	const bool carried = first % (unsigned long long)D != 0 && !(e.start == kTunerStartFresh && offset == 0);
	const int old = carried ? st.partial : 0;
	for (int lane = 0; lane < LANES; lane++)
		for (long long m = mFirst + lane; m < mEnd; m += LANES)
		{
			int d = TunerGroupSum(x, first, n, m, D);
			if (m == mFirst) d += old;
			ring[m & MASK] = d;
		}
	st.partial = (mEnd == mFirst ? old : 0) + TunerGroupSum(x, first, n, mEnd, D);
	st.gen = e.gen;
}

// TunerEvaluateKernel on one entry whose evaluation end lies in the piece
static TunerRecord Evaluate(const TunerEntry& e, const int* ring)
{
	const int W = e.window, top = e.maxLag + 1, L = W + e.maxLag + 2;
	std::vector<int> span((size_t)L);
	for (int i = 0; i < L; i++)
	{
		const long long m = e.evalM - (long long)(L - 1) + i;
		span[(size_t)i] = m < 0 ? 0 : ring[m & MASK];
	}
	std::vector<long long> r((size_t)top + 1);
	for (int tid = 0; tid < THREADS; tid++)
	{
		// (the kernel's form: a thread's lags side by side, a lag past the top summed as lag 0 and dropped; odd threads the plain form)
		int t[5];
		long long sum[5];
		for (int i = 0; i < 5; i++) t[i] = tid + i * THREADS <= top ? tid + i * THREADS : 0;
		if (tid % 2 == 0) TunerLagSums<5>(span.data(), L, W, t, sum);
		else
			for (int i = 0; i < 5; i++) sum[i] = TunerLagSum(span.data(), L, W, t[i]);
		for (int i = 0; i < 5; i++)
			if (tid + i * THREADS <= top) r[(size_t)(tid + i * THREADS)] = sum[i];
	}
	int zMin = INT_MAX, lagMin = INT_MAX;
	long long rmax = 0;
	for (int t = 1; t <= top; t++)
		if (r[(size_t)t] <= 0) zMin = std::min(zMin, t);
	const bool search = (unsigned long long)r[0] >= e.minEnergy && zMin != INT_MAX;
	if (search)
		for (int t = 1; t <= e.maxLag; t++)
			if (TunerIsCandidate(r[(size_t)t - 1], r[(size_t)t], r[(size_t)t + 1], t, zMin, e.minLag, e.maxLag)) rmax = std::max(rmax, r[(size_t)t]);
	if (search && rmax > 0)
		for (int t = 1; t <= e.maxLag; t++)
			if (TunerIsCandidate(r[(size_t)t - 1], r[(size_t)t], r[(size_t)t + 1], t, zMin, e.minLag, e.maxLag) && TunerPasses(r[(size_t)t], e.thresholdQ10, rmax))
				lagMin = std::min(lagMin, t);
	const int lag = lagMin == INT_MAX ? 0 : lagMin;
	TunerRecord rec;
	rec.row = e.row;
	rec.gen = e.gen;
	rec.reading.evaluations = e.evaluations;
	rec.reading.position = (e.evalM + 1) * (long long)e.decimation;
	rec.reading.e0 = (unsigned long long)r[0];
	for (int i = 0; i < 3; i++)
	{
		rec.reading.r[i] = lag > 0 ? r[(size_t)(lag - 1 + i)] : 0;
		rec.reading.e[i] = lag > 0 ? TunerSquareSum(span.data(), L, W, lag - 1 + i) : 0ull;
	}
	rec.reading.lag = lag;
	rec.reading.decimation = e.decimation;
	return rec;
}

int main()
{
	TunerBook book;
	book.Resize(ROWS);
	std::vector<TunerState> state(ROWS);
	std::vector<int> rings((size_t)ROWS * kTunerRingSamples, 0x55555555); // (nothing an evaluation reads was not written by its tuner)
	std::vector<TunerEntry> table(ROWS);
	int evaluating = 0;
	const auto entries = [&](bool call) {
		std::printf("E %d", book.NumEntries());
		for (int s = 0; s < ROWS; s++) std::printf(" %d", book.HasTuner(s) ? 1 : 0);
		std::printf(" |");
		for (int s = 0; s < ROWS; s++) std::printf(" %u", book.Gen(s));
		if (call) std::printf(" | %d", evaluating);
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
			TunerParams p;
			in >> row >> p.decimation >> p.windowSamples >> p.minLag >> p.maxLag >> p.hopSamples >> p.phase >> p.thresholdQ10 >> p.minEnergy;
			if (const char* why = TunerParamsError(p))
			{
				std::printf("! %s\n", why);
				continue;
			}
			book.Set(row, p);
			entries(false);
		}
		else if (cmd == "R" || cmd == "L")
		{
			int row;
			in >> row;
			if (cmd == "R") book.Remove(row);
			else book.Leave(row);
			entries(false);
		}
		else if (cmd == "A")
		{
			TunerRecord rec;
			in >> rec.row >> rec.gen >> rec.reading.evaluations;
			std::printf("A %d\n", book.Accept(rec) ? 1 : 0);
		}
		else if (cmd == "X")
		{
			size_t n;
			in >> n;
			std::vector<std::vector<float>> rows(ROWS, std::vector<float>(n));
			for (int s = 0; s < ROWS; s++)
			{
				std::getline(std::cin, line);
				std::istringstream row(line);
				std::string hex;
				for (size_t i = 0; i < n; i++)
				{
					row >> hex;
					rows[(size_t)s][i] = FromBits(hex);
				}
			}
			const int count = book.BuildTable(table.data(), (unsigned long long)n, &evaluating);
			std::vector<TunerRecord> records((size_t)evaluating);
			for (size_t done = 0; done < n; done += (size_t)kTunerPieceSamples)
			{
				const unsigned long long piece = std::min<size_t>((size_t)kTunerPieceSamples, n - done);
				for (int k = 0; k < count; k++)
					Append(table[(size_t)k], rows[(size_t)table[(size_t)k].row].data(), done, piece, state[(size_t)table[(size_t)k].row], &rings[(size_t)table[(size_t)k].row * kTunerRingSamples]);
				for (int k = 0; k < evaluating; k++)
				{
					const TunerEntry& e = table[(size_t)table[(size_t)k].evalEntry];
					const unsigned long long last = (unsigned long long)(e.evalM + 1) * (unsigned long long)e.decimation - 1ull;
					if (last < e.pos + done || last >= e.pos + done + piece) continue;
					records[(size_t)k] = Evaluate(e, &rings[(size_t)e.row * kTunerRingSamples]);
				}
			}
			book.Advance(n);
			for (const TunerRecord& rec : records) (void)book.Accept(rec);
			for (int k = 0; k < count; k++)
			{
				const int row = table[(size_t)k].row;
				const TunerReading g = book.HasReading(row) ? book.Latest(row) : TunerReading();
				std::printf("T %d %d %llu %lld %d %d %llu %lld %lld %lld %llu %llu %llu\n", row, book.HasReading(row) ? 1 : 0, g.evaluations, g.position, g.lag, g.decimation, g.e0,
					g.r[0], g.r[1], g.r[2], g.e[0], g.e[1], g.e[2]);
			}
			entries(true);
		}
		else return 2;
	}
	return 0;
}
