// tuner_stage.h -- the per-stream tuner stage of a batch: a pitch reading of the row a stream takes in, behind the
// meter's IN tap in front of the model launches (NA_BatchEnableTunerStage / NA_BatchSetStreamTuner / NA_BatchReadStreamTuner).  It never
// writes an audio row.  No reference counterpart: a host of the reference runs its tuner on the buffers it holds; here the rows stay on
// the device, and an evaluation is about a million multiply-adds.
//
// This header is the host bookkeeping, the table entry and the records the kernels read and write (tuner_stage_kernels.hip) and the
// functions both sides run: TunerQuantise (one sample), TunerGroupSum (one decimated sample), TunerLagSum(s) / TunerSquareSum (r[t], e[t])
// and the three tests of the selection.  It uses no HIP, so that it compiles and runs on its own.  All of it is index arithmetic on
// arrays sized on the set-up side (Resize): the real-time calls -- Set, Remove, Leave, BuildTable, Advance, Accept -- allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h).  Positions p = 0, 1, ... count the samples the caller sees on the stream's
// input row since the set call; D = decimation, W = windowSamples, H = hopSamples; W, the lags, H and phase count decimated samples.
//   c    = (x is NaN) ? 0 : min(max(x, -1.0f), 1.0f)
//   q[p] = (int) trunc(c * 32767.0f)                      (one f32 product, then integers only)
//   d[m] = q[mD] + q[mD+1] + ... + q[mD+D-1]   for m >= 0;   d[m] = 0 for m < 0        (|d| < 2^18)
//   evaluation k = 0, 1, ... ends at m_k = phase + (k+1)*H - 1 and belongs to the call that holds position (m_k+1)*D - 1
//   for t = 0 .. maxLag+1, signed / unsigned 64-bit:
//       r[t] = sum over j = 0 .. W-1 of d[m_k - j] * d[m_k - j - t]                      (|r| < 2^47)
//       e[t] = sum over j = 0 .. W-1 of d[m_k - j - t] * d[m_k - j - t]                  (e[0] = r[0])
//   lag = 0 if e[0] < minEnergy
//   z   = the smallest t in [1, maxLag+1] with r[t] <= 0;          none: lag = 0
//   candidates: t in [max(minLag, z+1), maxLag] with r[t] > 0 and r[t] > r[t-1] and r[t] >= r[t+1];   none: lag = 0
//   rmax = max of r[t] over the candidates
//   lag  = the smallest candidate t with 1024 * r[t] >= thresholdQ10 * rmax              (< 2^57)
// A reading holds evaluations = k + 1, position = (m_k + 1) * D, lag, decimation, e0 = e[0] and r[i], e[i] = r and e at lag - 1, lag,
// lag + 1 (all zero when lag = 0).  A call that holds several evaluation ends of a stream computes only the last of them;
// `evaluations` still counts them all.  Everything behind the one f32 product is an integer, so the bits of evaluation k do not depend
// on how the signal is cut into calls, on alignment or on stride.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_TUNER_HD __host__ __device__ __forceinline__
#define NA_TUNER_UNROLL(n) _Pragma(#n)
#else
#define NA_TUNER_HD inline
#define NA_TUNER_UNROLL(n)
#endif

namespace na
{
	constexpr int kTunerMaxDecimation = 8;
	constexpr int kTunerMinWindow = 32, kTunerMaxWindow = 2048;
	constexpr int kTunerMinMaxLag = 4, kTunerMaxLag = 1024;
	constexpr int kTunerMinHop = 16, kTunerMaxHop = 65536;
	constexpr int kTunerMinThreshold = 512, kTunerMaxThreshold = 1024;
	constexpr int kTunerMaxSpan = kTunerMaxWindow + kTunerMaxLag + 2; // the ring values an evaluation reads: d[m - W - maxLag - 1 .. m]
	constexpr int kTunerPieceSamples = 4096;                          // the longest run the stage appends at once
	// a row's ring of decimated samples: what an evaluation reads and, behind its end, the rest of the piece (at D = 1: a sample each)
	constexpr int kTunerRingSamples = 8192;
	static_assert(kTunerRingSamples >= kTunerMaxSpan + kTunerPieceSamples && (kTunerRingSamples & (kTunerRingSamples - 1)) == 0, "a power of two that holds a span and a piece");
	enum : int { kTunerStartNone = 0, kTunerStartFresh = 1 };

	// the constants of a tuner as the caller gives them (NA_TunerParams, field for field)
	struct TunerParams
	{
		int decimation = 2, windowSamples = 2048, minLag = 2, maxLag = 640, hopSamples = 1024, phase = 0, thresholdQ10 = 922, reserved = 0;
		unsigned long long minEnergy = 0;
	};

	// nullptr: fine; else the text of the first rule the constants break (it names the field)
	inline const char* TunerParamsError(const TunerParams& p)
	{
		if (p.decimation < 1 || p.decimation > kTunerMaxDecimation) return "decimation must lie in [1, 8]";
		if (p.windowSamples < kTunerMinWindow || p.windowSamples > kTunerMaxWindow) return "windowSamples must lie in [32, 2048]";
		if (p.maxLag < kTunerMinMaxLag || p.maxLag > kTunerMaxLag) return "maxLag must lie in [4, 1024]";
		if (p.minLag < 2 || p.minLag > p.maxLag) return "minLag must lie in [2, maxLag]";
		if (p.hopSamples < kTunerMinHop || p.hopSamples > kTunerMaxHop) return "hopSamples must lie in [16, 65536]";
		if (p.phase < 0 || p.phase >= p.hopSamples) return "phase must lie in [0, hopSamples)";
		if (p.thresholdQ10 < kTunerMinThreshold || p.thresholdQ10 > kTunerMaxThreshold) return "thresholdQ10 must lie in [512, 1024]";
		return nullptr;
	}

	// a tuner's newest evaluation (NA_TunerReading, field for field; 80 bytes)
	struct TunerReading
	{
		unsigned long long evaluations = 0;
		long long position = 0;
		long long r[3] = { 0, 0, 0 };
		unsigned long long e0 = 0, e[3] = { 0, 0, 0 };
		int lag = 0, decimation = 0;
	};

	// One unit of work of the stage's launches: a row and its tuner (72 bytes).  `pos` is the position of the call's first sample;
	// `start`: that is position 0 of a tuner set since the last call, whatever the row's state holds is not this tuner's (no memset
	// travels with a set call).  `gen` is echoed in the record an evaluation produces.  evalM >= 0: the call holds evaluation ends of
	// the tuner, the last of them at decimated sample evalM, and with it `evaluations` of them have gone by.  evalEntry is not the
	// entry's own: slot k of the table holds in it the index of the k-th entry that evaluates in this call (BuildTable).
	struct TunerEntry
	{
		int row = -1;
		int decimation = 0, window = 0, minLag = 0, maxLag = 0, thresholdQ10 = 0;
		int start = kTunerStartNone;
		uint32_t gen = 0;
		unsigned long long pos = 0;
		unsigned long long minEnergy = 0;
		long long evalM = -1;
		unsigned long long evaluations = 0;
		int evalEntry = -1;
		int reserved = 0;
	};

	// per row, on the device (8 bytes): the group of D samples that straddles two calls.  How many samples it holds is pos mod D.
	struct TunerState
	{
		int partial = 0;
		uint32_t gen = 0;
	};

	// what an evaluation leaves, and the result copy brings to the host (88 bytes)
	struct TunerRecord
	{
		int row = -1;
		uint32_t gen = 0;
		TunerReading reading;
	};

	// one sample: the first two lines of the contract.  The comparisons are ordered ones, so a NaN falls through both and is caught by
	// its bit pattern; whether the product of a subnormal is flushed or not, it truncates to 0.
	NA_TUNER_HD int TunerQuantise(float x)
	{
		uint32_t b;
		__builtin_memcpy(&b, &x, 4);
		if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0;
		const float c = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
		return (int)(c * 32767.0f);
	}

	// the part of group m -- positions [mD, mD + D) -- that lies in the run x[0 .. n) whose first sample is position `first`
	NA_TUNER_HD int TunerGroupSum(const float* x, unsigned long long first, unsigned long long n, long long m, int D)
	{
		const unsigned long long lo = (unsigned long long)m * (unsigned long long)D, hi = lo + (unsigned long long)D;
		const unsigned long long from = lo > first ? lo : first, to = hi < first + n ? hi : first + n;
		int sum = 0;
		for (unsigned long long p = from; p < to; p++) sum += TunerQuantise(x[p - first]);
		return sum;
	}

	// The evaluation's view of the ring: span[i], i = 0 .. L-1 with L = W + maxLag + 2, is d[m_k - (L-1) + i], oldest first -- zero where
	// that index is negative.  r[t] and e[t] of the contract over it:
	NA_TUNER_HD long long TunerLagSum(const int* span, int L, int W, int t)
	{
		long long sum = 0;
		for (int j = 0; j < W; j++) sum += (long long)span[L - 1 - j] * (long long)span[L - 1 - j - t];
		return sum;
	}
	// r[] of N lags at once, t[0 .. N): the d[m - j] read is shared and the N chains of multiply-adds are independent of each other
	template <int N>
	NA_TUNER_HD void TunerLagSums(const int* span, int L, int W, const int* t, long long* sum)
	{
		long long acc[N];
		for (int i = 0; i < N; i++) acc[i] = 0;
		NA_TUNER_UNROLL(unroll 4)
		for (int j = 0; j < W; j++)
		{
			const long long a = span[L - 1 - j];
			NA_TUNER_UNROLL(unroll)
			for (int i = 0; i < N; i++) acc[i] += a * (long long)span[L - 1 - j - t[i]];
		}
		for (int i = 0; i < N; i++) sum[i] = acc[i];
	}
	NA_TUNER_HD unsigned long long TunerSquareSum(const int* span, int L, int W, int t)
	{
		unsigned long long sum = 0;
		for (int j = 0; j < W; j++)
		{
			const long long v = span[L - 1 - j - t];
			sum += (unsigned long long)(v * v);
		}
		return sum;
	}
	// the selection's tests, lag by lag (z: the first t >= 1 with r[t] <= 0)
	NA_TUNER_HD bool TunerIsCandidate(long long before, long long at, long long after, int t, int z, int minLag, int maxLag)
	{
		return t >= minLag && t > z && t <= maxLag && at > 0 && at > before && at >= after;
	}
	NA_TUNER_HD bool TunerPasses(long long at, int thresholdQ10, long long rmax) { return 1024 * at >= (long long)thresholdQ10 * rmax; }

	class TunerBook
	{
	public:
		// set-up side: tables for `rows` rows (existing rows keep what they have)
		void Resize(int rowCount)
		{
			if (rowCount > (int)rows.size()) rows.resize((size_t)rowCount);
		}
		int Rows() const { return (int)rows.size(); }

		// ---- real-time side ----
		bool HasEntries() const { return numEntries > 0; }
		int NumEntries() const { return numEntries; }
		bool HasTuner(int s) const { return rows[(size_t)s].has; }
		const TunerParams& Params(int s) const { return rows[(size_t)s].params; }
		uint32_t Gen(int s) const { return rows[(size_t)s].gen; }
		unsigned long long Position(int s) const { return rows[(size_t)s].pos; }
		bool HasReading(int s) const { return rows[(size_t)s].has && rows[(size_t)s].arrived; }
		const TunerReading& Latest(int s) const { return rows[(size_t)s].latest; }

		// p: valid (TunerParamsError).  The tuner starts -- or starts again -- at the next sample, at position 0, under a new generation:
		// nothing an earlier tuner of the row produced is read from here on
		void Set(int s, const TunerParams& p)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				r.has = true;
				numEntries++;
			}
			r.pos = 0;
			r.gen = ++lastGen;
			r.arrived = false;
			r.params = p;
			r.params.reserved = 0;
		}
		// the tuner goes at once: it touches no audio, so there is no tail
		void Remove(int s)
		{
			Row& r = rows[(size_t)s];
			if (!r.has) return;
			r = Row();
			r.gen = ++lastGen;
			numEntries--;
		}
		// park / removal of the stream: the same
		void Leave(int s) { Remove(s); }

		// evaluation ends at or before decimated sample count `have` (= the decimated samples complete so far)
		static unsigned long long EndsBy(const TunerParams& p, unsigned long long have)
		{
			return have >= (unsigned long long)p.phase ? (have - (unsigned long long)p.phase) / (unsigned long long)p.hopSamples : 0ull;
		}

		// the entries of the next call of n samples, into table[0 .. NumEntries()); returns how many.  *evaluating: how many of them hold
		// an evaluation end in the call; their indices are in table[0 .. *evaluating).evalEntry
		int BuildTable(TunerEntry* table, unsigned long long n, int* evaluating) const
		{
			int count = 0, evals = 0;
			*evaluating = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				const TunerParams& p = r.params;
				TunerEntry& e = table[count];
				e.row = (int)s;
				e.decimation = p.decimation;
				e.window = p.windowSamples;
				e.minLag = p.minLag;
				e.maxLag = p.maxLag;
				e.thresholdQ10 = p.thresholdQ10;
				e.start = r.pos == 0 ? kTunerStartFresh : kTunerStartNone;
				e.gen = r.gen;
				e.pos = r.pos;
				e.minEnergy = p.minEnergy;
				const unsigned long long D = (unsigned long long)p.decimation;
				const unsigned long long before = EndsBy(p, r.pos / D), after = EndsBy(p, (r.pos + n) / D);
				e.evalM = after > before ? (long long)((unsigned long long)p.phase + after * (unsigned long long)p.hopSamples) - 1 : -1;
				e.evaluations = after;
				e.evalEntry = -1;
				e.reserved = 0;
				if (after > before) table[evals++].evalEntry = count; // (evals <= count: slot `evals` has been filled in already, or is this one)
				count++;
			}
			*evaluating = evals;
			return count;
		}

		// `n` samples were taken with the table BuildTable made
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
				if (r.has) r.pos += n;
		}

		// a record has arrived on the host: it becomes the row's newest reading if it is this tuner's (the generations agree) and holds
		// an evaluation; true: taken
		bool Accept(const TunerRecord& rec)
		{
			if (rec.row < 0 || rec.row >= (int)rows.size()) return false;
			Row& r = rows[(size_t)rec.row];
			if (!r.has || r.gen != rec.gen || rec.reading.evaluations == 0) return false;
			r.latest = rec.reading;
			r.arrived = true;
			return true;
		}

	private:
		struct Row
		{
			bool has = false, arrived = false;
			uint32_t gen = 0;
			unsigned long long pos = 0; // samples the tuner has taken
			TunerParams params;
			TunerReading latest;
		};
		std::vector<Row> rows;
		int numEntries = 0;
		uint32_t lastGen = 0; // of the batch: a generation is never used twice (2^32 set calls apart)
	};

	// (tuner_stage_kernels.hip) one piece of a call: samples [offset, offset + n) of the call, n <= kTunerPieceSamples, of every entry's
	// row (`rows` points at the call's first sample; rows `stride` floats apart).  The append launch runs over table[0 .. count); the
	// evaluate launch over the `evaluating` entries listed in table[..].evalEntry, of which those whose evaluation end lies in the piece
	// write results[list slot].
	struct TunerLaunch
	{
		const TunerEntry* table;
		int count, evaluating;
		const float* rows;
		long stride;
		unsigned long long offset, n;
		TunerState* state;
		int* rings; // [rows][kTunerRingSamples]
		TunerRecord* results;
	};

	unsigned long long TunerStageLaunches(); // launches of the stage's two kernels so far (NA_DebugTunerLaunches)

	// ---- host helpers (double precision; not part of the exact contract) ----
	// hz and clarity of a reading: a parabola through the normalised r at lag - 1, lag, lag + 1.  false (hz = clarity = 0): lag == 0
	inline bool TunerPitch(const TunerReading& g, double sampleRate, double& hz, double& clarity)
	{
		hz = clarity = 0.0;
		if (g.lag <= 0 || g.decimation <= 0) return false;
		double n[3];
		for (int i = 0; i < 3; i++)
		{
			const double den = (double)g.e0 + (double)g.e[i];
			n[i] = den != 0.0 ? 2.0 * (double)g.r[i] / den : 0.0;
		}
		const double den = n[0] - 2.0 * n[1] + n[2];
		const double off = den < 0.0 ? std::min(1.0, std::max(-1.0, 0.5 * (n[0] - n[2]) / den)) : 0.0;
		hz = sampleRate / ((double)g.decimation * ((double)g.lag + off));
		clarity = n[1] - 0.25 * (n[0] - n[2]) * off;
		return true;
	}

	// the constants for a range of notes; nullptr: fine, else what is wrong
	inline const char* TunerParamsFromRange(double sampleRate, double lowestHz, double highestHz, double evaluationsPerSecond, TunerParams& out)
	{
		if (!(sampleRate > 0.0) || !std::isfinite(sampleRate)) return "sampleRate must be finite and > 0";
		if (!(lowestHz > 0.0) || !std::isfinite(highestHz) || !(highestHz >= lowestHz)) return "0 < lowestHz <= highestHz required";
		if (!(evaluationsPerSecond > 0.0) || !std::isfinite(evaluationsPerSecond)) return "evaluationsPerSecond must be finite and > 0";
		int D = 1;
		for (int d = 1; d <= kTunerMaxDecimation; d++)
			if (sampleRate / (d * highestHz) >= 16.0) D = d;
		const double maxLag = std::ceil(sampleRate / (D * lowestHz)) + 2.0;
		if (maxLag > (double)kTunerMaxLag) return "lowestHz needs a maxLag above 1024";
		TunerParams p;
		p.decimation = D;
		p.maxLag = (int)maxLag;
		p.minLag = std::max(2, (int)std::floor(sampleRate / (D * highestHz)) - 1);
		p.windowSamples = std::min(kTunerMaxWindow, std::max(kTunerMinWindow, 3 * p.maxLag));
		const double hop = std::floor(sampleRate / (D * evaluationsPerSecond) + 0.5);
		if (hop > (double)kTunerMaxHop) return "evaluationsPerSecond needs a hopSamples above 65536";
		p.hopSamples = std::max(kTunerMinHop, (int)hop);
		p.phase = 0;
		p.thresholdQ10 = 922;
		p.reserved = 0;
		p.minEnergy = (unsigned long long)p.windowSamples * (unsigned long long)(33 * D) * (unsigned long long)(33 * D);
		if (const char* why = TunerParamsError(p)) return why; // (a range no tuner of these limits covers)
		out = p;
		return nullptr;
	}
}
