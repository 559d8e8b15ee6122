// limiter_stage.h -- the per-stream limiter stage of a batch: a feed-forward look-ahead brickwall limiter on the row
// the caller receives, behind the mix stage and in front of the meter's OUT tap (NA_BatchEnableLimiterStage /
// NA_BatchSetStreamLimiter).  No reference counterpart: a host of the reference runs its safety limiter on the buffers it holds; here
// the rows stay on the device.
//
// This header is the host bookkeeping, the table entry the kernel reads (limiter_stage_kernels.hip) and the per-sample functions both
// sides evaluate.  It uses no HIP, so that it compiles and runs on its own.  All of it is index arithmetic on arrays sized on the
// set-up side (Resize): the real-time calls -- Set, Remove, Leave, BuildTable, Advance -- allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h): every floating-point operation is one separately rounded f32 operation,
// round to nearest even, no FMA contraction, subnormals kept; the quotient is correctly rounded.  L = lookahead, H = hold.  Positions
// t = 0, 1, ... count the samples of the row since the set call that created the entry; k = t - (the position of the LAST set call).
//   c[t]    = from for k < 0, to for k >= R - 1, else fl(from + fl(fl(to - from) * w)), w = (float)(k + 1) / (float)R
//   need[t] = |x[t]| > c[t] ? fl(c[t] / |x[t]|) : 1                       (t < 0: need = 1 and x = +0, by position)
//   m[t]    = min(need[t - L - H .. t])
//   S_1[t]  = fl(m[t - 1] + m[t]);  S_(j+1)[t] = fl(S_j[t - 2^j] + S_j[t]);  S = S_(log2 L): the pairwise tree over m[t - L + 1 .. t]
//   g[t]    = fl(S[t] * (1 / L))                                          (a power of two: exact unless it ends subnormal)
//   y[t]    = min(max(fl(x[t - L] * g[t]), -c[t]), c[t])
// Every output between two set calls is that of the earlier one's (from, to, R) and H, which reach back over the 2 L + H samples the
// output reads; k is advanced by whole calls and never accumulated.  The kernel recomputes need, m and S of the samples behind a call
// from the 2 L + H INPUT samples the stage keeps per row, so a sample's bits do not depend on how the signal is cut into calls, on
// the stride or on the other streams.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_LIM_HD __host__ __device__ __forceinline__
#else
#define NA_LIM_HD inline
#endif

namespace na
{
	constexpr int kLimMinLookahead = 8, kLimMaxLookahead = 512; // L: a power of two, the stage's latency in samples
	constexpr int kLimMaxHold = 4096;                           // H
	constexpr int kLimHistory = 2 * kLimMaxLookahead + kLimMaxHold; // the input samples the stage keeps per row: a ring of 5120 floats, 20 KB
	constexpr int kLimPieceSamples = 1024;                      // the longest run one launch processes; longer calls run in pieces
	constexpr int kLimMaxRamp = 1 << 20;

	// the constants of a limiter as the caller gives them (NA_LimiterParams, field for field)
	struct LimiterParams
	{
		int lookahead = 64, hold = 0;
		float ceiling = 1.0f;
		int reserved = 0;
	};

	inline int LimLog2(int L)
	{
		int p = 0;
		while ((1 << (p + 1)) <= L) p++;
		return p;
	}

	// nullptr: fine; else the text of the first rule the constants break (it names the field)
	inline const char* LimiterParamsError(const LimiterParams& p)
	{
		if (p.lookahead < kLimMinLookahead || p.lookahead > kLimMaxLookahead || (p.lookahead & (p.lookahead - 1)) != 0) return "lookahead must be a power of two in [8, 512]";
		if (p.hold < 0 || p.hold > kLimMaxHold) return "hold must lie in [0, 4096]";
		if (!std::isfinite(p.ceiling) || !(p.ceiling > 0.0f)) return "ceiling must be finite and greater than 0";
		return nullptr;
	}

	// NA_LimiterParamsFromDb: host arithmetic in double, each value rounded once.  ceiling = 10^(ceilingDb / 20); lookahead = the power
	// of two in [8, 512] nearest to lookaheadMs * rate / 1000 (v <= 1.5 P picks P); hold = round(holdMs * rate / 1000).
	// nullptr: fine; else what is wrong.
	inline const char* LimiterParamsFromDb(int sampleRate, double ceilingDb, double lookaheadMs, double holdMs, LimiterParams& out)
	{
		if (sampleRate < 1) return "sampleRate must be >= 1";
		if (!std::isfinite(ceilingDb)) return "ceiling must be finite and greater than 0";
		if (!std::isfinite(lookaheadMs) || lookaheadMs < 0.0) return "lookahead must be a power of two in [8, 512]";
		if (!std::isfinite(holdMs) || holdMs < 0.0) return "hold must lie in [0, 4096]";
		LimiterParams p;
		p.ceiling = (float)std::pow(10.0, ceilingDb / 20.0);
		const double v = lookaheadMs * (double)sampleRate / 1000.0;
		p.lookahead = kLimMinLookahead;
		while (p.lookahead < kLimMaxLookahead && v > 1.5 * (double)p.lookahead) p.lookahead *= 2;
		p.hold = (int)std::min(std::floor(holdMs * (double)sampleRate / 1000.0 + 0.5), 2147483647.0);
		if (const char* why = LimiterParamsError(p)) return why;
		out = p;
		return nullptr;
	}

	// c of the sample k samples behind the last set call (k < 0: in front of it)
	NA_LIM_HD float LimCeilingAt(float from, float to, int R, long long k)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (k < 0) return from;
		if (k >= (long long)R - 1) return to;
		const float w = (float)(k + 1) / (float)R;
		const float span = to - from;
		const float part = span * w;
		return from + part;
	}

	// need of a sample under ceiling c
	NA_LIM_HD float LimNeed(float x, float c)
	{
		const float a = fabsf(x);
		return a > c ? c / a : 1.0f;
	}

	// y of a delayed sample under gain sum S (of L values, invL = 1 / L) and ceiling c
	NA_LIM_HD float LimOutput(float xDelayed, float S, float invL, float c)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float g = S * invL;
		const float v = xDelayed * g;
		return fminf(fmaxf(v, -c), c);
	}

	// One unit of work of the stage's launch (48 bytes): a row and where the call begins.  `held`: the input samples of this entry the
	// ring holds in front of the call's first sample, saturating at kLimHistory -- a read further back yields need = 1 and x = +0 by
	// comparing positions, never by what the ring holds (no memset travels with a set call).  `ringPos`: where the call's first sample
	// goes in the row's ring.  `done`: samples since the last set call, at the call's first sample.
	struct LimiterEntry
	{
		int row = -1, lookahead = 0, logL = 0, hold = 0, R = 0;
		int held = 0, ringPos = 0, reserved = 0;
		long long done = 0;
		float from = 1.0f, to = 1.0f;
	};
	static_assert(sizeof(LimiterEntry) == 48, "the entry the kernel reads");

	class LimiterBook
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
		bool HasLimiter(int s) const { return rows[(size_t)s].has; }
		const LimiterParams& Target(int s) const { return rows[(size_t)s].params; }
		// p: valid (LimiterParamsError), lookahead that of the entry if there is one.  A new entry starts at the next sample, at
		// position 0, at p's ceiling (nothing to ramp from); an entry's ceiling ramps from that of the last sample produced
		void Set(int s, const LimiterParams& p, int rampSamples)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				r = Row();
				r.has = true;
				numEntries++;
				r.from = p.ceiling;
				rampSamples = 0;
			}
			else
				r.from = LimCeilingAt(r.from, r.to, r.R, r.done - 1);
			r.to = p.ceiling;
			r.R = rampSamples;
			r.done = 0;
			r.params = p;
			r.params.reserved = 0;
		}
		// the limiter goes at once, with its history: the row comes out undelayed from the next call on
		void Remove(int s)
		{
			Row& r = rows[(size_t)s];
			if (!r.has) return;
			r = Row();
			numEntries--;
		}
		// park / removal of the stream: the same
		void Leave(int s) { Remove(s); }

		// the entries of the next call, into table[0 .. NumEntries()); returns how many, and the largest 2 L + H and L among them (what
		// the launch sizes its LDS by)
		int BuildTable(LimiterEntry* table, int& maxWindow, int& maxLookahead) const
		{
			int count = 0;
			maxWindow = maxLookahead = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				LimiterEntry& e = table[count++];
				e = LimiterEntry();
				e.row = (int)s;
				e.lookahead = r.params.lookahead;
				e.logL = LimLog2(r.params.lookahead);
				e.hold = r.params.hold;
				e.R = r.R;
				e.held = r.held;
				e.ringPos = r.ringPos;
				e.done = r.done;
				e.from = r.from;
				e.to = r.to;
				maxWindow = std::max(maxWindow, 2 * e.lookahead + e.hold);
				maxLookahead = std::max(maxLookahead, e.lookahead);
			}
			return count;
		}

		// `n` samples were taken with the table BuildTable made
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				r.ringPos = (int)(((unsigned long long)r.ringPos + n) % (unsigned long long)kLimHistory);
				r.held = (int)std::min<unsigned long long>((unsigned long long)kLimHistory, (unsigned long long)r.held + n);
				r.done += (long long)n;
			}
		}

	private:
		struct Row
		{
			bool has = false;
			int R = 0, held = 0, ringPos = 0;
			long long done = 0; // samples since the last set call
			float from = 1.0f, to = 1.0f;
			LimiterParams params;
		};
		std::vector<Row> rows;
		int numEntries = 0;
	};

	// (limiter_stage_kernels.hip) the launch of one piece over `count` entries of the device table: `n` samples of every entry's row
	// from sample `done` of the call on, rows `stride` floats apart, in place; history: [rowCapacity][kLimHistory]; maxWindow, maxLookahead:
	// the largest 2 L + H and L among the entries (the launch's LDS)
	struct LimiterLaunch
	{
		const LimiterEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long done;
		int n;
		float* history;
		int rowCapacity;
		int maxWindow, maxLookahead;
	};

	unsigned long long LimiterStageLaunches(); // launches of the stage's kernel so far (NA_DebugLimiterLaunches)
}
