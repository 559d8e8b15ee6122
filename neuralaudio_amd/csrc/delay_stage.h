// delay_stage.h -- the per-stream delay stage of a batch: an echo -- a feedback delay line with a one-pole low-pass and a
// one-pole high-pass in the loop -- on the row of every stream that has one, behind the cabinet stage and in front of the reverb stage
// (NA_BatchEnableDelayStage / NA_BatchSetStreamDelay).  No reference counterpart: a host of the reference runs its delay on the buffer
// it holds; here the rows stay on the device.
//
// This header is the host bookkeeping, the table entry the kernel reads (delay_stage_kernels.hip) and the ONE step function both sides
// run.  It uses no HIP, so that it compiles and runs on its own.  All of it is index arithmetic on arrays sized on the set-up side
// (Configure, Resize): the real-time calls -- Set, Leave, BuildTable, Advance -- allocate nothing.
//
// Unlike the feed-forward stages this one feeds back through a long memory: sample t depends on sample t - D of the stage's own line w,
// which lives in a ring per row on the device, with the two filter states l and q.  The host mirror counts positions: where the next
// sample goes in the ring (pos), how many samples the line holds (hist, saturating at maxDelaySamples) -- a read in front of T0 yields +0
// by comparing positions, never by what the ring holds, so nothing is cleared on the device -- and where a fade stands (k).
//
// Arithmetic (the contract of include/neuralaudio_amd.h): separately rounded f32 operations in this order, no FMA contraction, f32
// subnormals kept (DelayStep below, compiled with contraction off).  Constants of a setting: D = delaySamples, fb = feedback,
// aL = lowpassCoeff, aH = highpassCoeff, wet, dry.  State: the line w, f32 l and q.  Per sample, x the row's sample:
//   x' = isnan(x) ? 0 : clamp(x, +-1e18f)
//   d  = w[t - D]                                       (+0 where t - D < 0)
//   l  = (aL == 1) ? d : fl(l + fl(aL * fl(d - l)))     (aL == 1: l takes d, bit for bit)
//   if aH == 0: h = l, q left alone;  else: q = fl(q + fl(aH * fl(l - q))), h = fl(l - q)
//   w[t] = clamp(fl(x' + fl(fb * h)), +-1e30f)
//   y  = (wet == 0) ? fl(dry * x') : fl(fl(dry * x') + fl(wet * h))
// During a fade from setting A to setting B (length N, k samples since the set call, wk = OutStageWeightAt(N, k)): aL and aH are B's;
// fb, wet and dry are B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk)); if D_A != D_B, d is w[t - D_B] where wk == 1, else
// fl(fl(fl(1 - wk) * w[t - D_A]) + fl(wk * w[t - D_B])).  "No delay" as A or as B is the other setting with wet = 0, dry = 1.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "output_stage.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_DELAY_HD __host__ __device__ __forceinline__
#else
#define NA_DELAY_HD inline
#endif

namespace na
{
	constexpr int kDelayMaxSamples = 1 << 18;  // maxDelaySamples
	constexpr int kDelayPieceSamples = 2048;   // the longest run one launch processes; longer calls run in pieces
	constexpr float kDelayMaxFeedback = 0.99f; // |feedback|
	constexpr float kDelayMaxMix = 1e6f;       // |wet|, |dry|

	// the constants of a delay as the caller gives them (NA_DelayParams)
	struct DelayParams
	{
		int delaySamples = 1;
		float feedback = 0.0f, lowpassCoeff = 1.0f, highpassCoeff = 0.0f, wet = 0.0f, dry = 1.0f;
	};

	// nullptr: fine; else the text of the first rule the constants break (it names the field).  delaySamples is held against
	// `maxDelaySamples`, the batch's or -- without a batch -- the largest a batch can have.
	inline const char* DelayParamsError(const DelayParams& p, int maxDelaySamples)
	{
		if (p.delaySamples < 1 || p.delaySamples > maxDelaySamples)
			return "delaySamples must lie in [1, maxDelaySamples]";
		if (!std::isfinite(p.feedback) || std::fabs(p.feedback) > kDelayMaxFeedback) return "feedback must lie in [-0.99, 0.99]";
		if (!std::isfinite(p.lowpassCoeff) || !(p.lowpassCoeff > 0.0f) || p.lowpassCoeff > 1.0f) return "lowpassCoeff must lie in (0, 1]";
		if (!std::isfinite(p.highpassCoeff) || p.highpassCoeff < 0.0f || !(p.highpassCoeff < 1.0f)) return "highpassCoeff must lie in [0, 1)";
		if (!std::isfinite(p.wet) || std::fabs(p.wet) > kDelayMaxMix) return "wet must be finite and at most 1e6 in magnitude";
		if (!std::isfinite(p.dry) || std::fabs(p.dry) > kDelayMaxMix) return "dry must be finite and at most 1e6 in magnitude";
		return nullptr;
	}

	// NA_DelayParamsFromMs: host arithmetic in double, rounded once.  delaySamples = max(1, round(ms * rate / 1000)); lowpassCoeff = 1 when
	// highCutHz <= 0 or >= rate / 2, else 1 - exp(-2 pi highCutHz / rate); highpassCoeff = 0 when lowCutHz <= 0, else
	// 1 - exp(-2 pi lowCutHz / rate); wet = 10^(wetDb / 20) with -inf -> 0, dry likewise.  nullptr: fine; else what is wrong.
	inline const char* DelayParamsFromMs(int sampleRate, double delayMs, double feedback, double lowCutHz, double highCutHz, double wetDb, double dryDb, DelayParams& out)
	{
		if (sampleRate < 1) return "sampleRate must be >= 1";
		if (!std::isfinite(delayMs) || delayMs < 0.0) return "delaySamples must lie in [1, maxDelaySamples]";
		if (!std::isfinite(feedback)) return "feedback must lie in [-0.99, 0.99]";
		if (!std::isfinite(highCutHz)) return "lowpassCoeff must lie in (0, 1]";
		if (!std::isfinite(lowCutHz)) return "highpassCoeff must lie in [0, 1)";
		if (std::isnan(wetDb) || wetDb == INFINITY) return "wet must be finite and at most 1e6 in magnitude";
		if (std::isnan(dryDb) || dryDb == INFINITY) return "dry must be finite and at most 1e6 in magnitude";
		const double rate = (double)sampleRate;
		const double twoPi = 6.283185307179586476925286766559;
		DelayParams p;
		p.delaySamples = (int)std::min(std::max(1.0, std::floor(delayMs * rate / 1000.0 + 0.5)), 2147483647.0);
		p.feedback = (float)feedback;
		p.lowpassCoeff = (highCutHz <= 0.0 || highCutHz >= rate / 2.0) ? 1.0f : (float)(1.0 - std::exp(-twoPi * highCutHz / rate));
		p.highpassCoeff = lowCutHz <= 0.0 ? 0.0f : (float)(1.0 - std::exp(-twoPi * lowCutHz / rate));
		p.wet = wetDb == -INFINITY ? 0.0f : (float)std::pow(10.0, wetDb / 20.0);
		p.dry = dryDb == -INFINITY ? 0.0f : (float)std::pow(10.0, dryDb / 20.0);
		if (const char* why = DelayParamsError(p, kDelayMaxSamples)) return why;
		out = p;
		return nullptr;
	}

	// One unit of work of the stage's launch: a row, the two settings of its fade (equal outside one) and where the call begins.
	struct DelayEntry
	{
		int row = -1;
		int DA = 1, DB = 1;          // the read heads: the setting it fades from, the one it has (fades to)
		int N = 0, k = 0;            // the fade: its length and the samples produced since the set call (0, 0: none)
		float fbA = 0.0f, fbB = 0.0f, wetA = 0.0f, wetB = 0.0f, dryA = 1.0f, dryB = 1.0f;
		float aL = 1.0f, aH = 0.0f;  // the filters: B's from k = 0
		unsigned pos = 0;            // where the call's first sample goes in the row's ring
		int hist = 0;                // samples the line holds in front of the call (saturating at maxDelaySamples: enough for any D)
		int start = 0;               // T0 lies in front of this call: l = q = 0 instead of the stored state (no memset travels with a set call)
		int toNone = 0;              // a fade to no delay: the entry retires with the sample at which the fade ends, later ones are not touched
	};
	static_assert(sizeof(DelayEntry) == 68, "an entry is seventeen words");

	// per row, on the device (8 bytes)
	struct DelayFilter
	{
		float l = 0.0f, q = 0.0f;
	};

	// fb, wet, dry of a sample: B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk))
	NA_DELAY_HD float DelayRamp(float gA, float gB, float wk)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (wk == 1.0f) return gB;
		const float span = gB - gA;
		const float part = span * wk;
		return gA + part;
	}

	NA_DELAY_HD float DelayClamp(float v, float limit) { return fminf(fmaxf(v, -limit), limit); }

	// one sample: the contract above, line by line.  wk: the fade's weight at this sample (1 outside a fade); dA = w[t - D_A],
	// dB = w[t - D_B] (+0 in front of T0; dA is read only where the heads differ and wk < 1).  Returns y; `w` is what goes into the line.
	NA_DELAY_HD float DelayStep(const DelayEntry& e, DelayFilter& s, float wk, float x, float dA, float dB, float& w)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float xs = (x != x) ? 0.0f : DelayClamp(x, 1e18f);
		float d = dB;
		if (wk != 1.0f && e.DA != e.DB)
		{
			const float rest = 1.0f - wk;
			const float partA = rest * dA;
			const float partB = wk * dB;
			d = partA + partB;
		}
		const float fb = DelayRamp(e.fbA, e.fbB, wk);
		const float wet = DelayRamp(e.wetA, e.wetB, wk);
		const float dry = DelayRamp(e.dryA, e.dryB, wk);
		if (e.aL == 1.0f) s.l = d;
		else
		{
			const float dl = d - s.l;
			const float step = e.aL * dl;
			s.l = s.l + step;
		}
		float h = s.l;
		if (e.aH != 0.0f)
		{
			const float lq = s.l - s.q;
			const float step = e.aH * lq;
			s.q = s.q + step;
			h = s.l - s.q;
		}
		const float back = fb * h;
		const float sum = xs + back;
		w = DelayClamp(sum, 1e30f);
		const float direct = dry * xs;
		if (wet == 0.0f) return direct;
		const float echo = wet * h;
		return direct + echo;
	}

	class DelayBook
	{
	public:
		// ---- set-up side ----
		// the smallest power of two that holds the longest delay and a piece
		static int RingFor(int maxDelay)
		{
			int ring = 1;
			while (ring < maxDelay + kDelayPieceSamples) ring *= 2;
			return ring;
		}
		void Configure(int maxDelay)
		{
			maxDelaySamples = maxDelay;
			ringSamples = RingFor(maxDelay);
		}
		void Resize(int rowCount)
		{
			if (rowCount > (int)rows.size()) rows.resize((size_t)rowCount);
		}
		int Rows() const { return (int)rows.size(); }
		int MaxDelay() const { return maxDelaySamples; }
		int RingSamples() const { return ringSamples; }

		// ---- real-time side ----
		bool HasEntries() const { return numEntries > 0; }
		int NumEntries() const { return numEntries; }
		// a delay that is not fading to none
		bool HasDelay(int s) const { return rows[(size_t)s].has && !rows[(size_t)s].toNone; }
		bool IsEntry(int s) const { return rows[(size_t)s].has; }
		const DelayParams& Target(int s) const { return rows[(size_t)s].B; }
		bool Fading(int s) const { return rows[(size_t)s].fading; }
		int FadeRemaining(int s) const { return rows[(size_t)s].fading ? rows[(size_t)s].N - rows[(size_t)s].k : 0; }

		// s: in no fade; p: valid (DelayParamsError) or nullptr: no delay; N >= 0
		void Set(int s, const DelayParams* p, int N)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				if (!p) return;
				// T0: the line and the filters start with the next sample
				r = Row();
				r.has = true;
				r.start = true;
				numEntries++;
				r.B = *p;
				r.A = Silent(*p);
			}
			else
			{
				r.A = r.B;
				r.B = p ? *p : Silent(r.A);
				r.toNone = p == nullptr;
			}
			if (N > 0)
			{
				r.fading = true;
				r.N = N;
				r.k = 0;
				return;
			}
			r.A = r.B;
			if (r.toNone) Retire(r);
		}
		// park / removal: no delay at once, the history is dropped
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (r.has) Retire(r);
		}

		// the entries of the next call, into table[0 .. NumEntries()); returns how many
		int BuildTable(DelayEntry* table) const
		{
			int count = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				DelayEntry& e = table[count++];
				e.row = (int)s;
				e.DA = r.A.delaySamples;
				e.DB = r.B.delaySamples;
				e.N = r.fading ? r.N : 0;
				e.k = r.fading ? r.k : 0;
				e.fbA = r.A.feedback;
				e.fbB = r.B.feedback;
				e.wetA = r.A.wet;
				e.wetB = r.B.wet;
				e.dryA = r.A.dry;
				e.dryB = r.B.dry;
				e.aL = r.B.lowpassCoeff;
				e.aH = r.B.highpassCoeff;
				e.pos = r.pos;
				e.hist = r.hist;
				e.start = r.start ? 1 : 0;
				e.toNone = r.toNone ? 1 : 0;
			}
			return count;
		}

		// `n` samples were produced with the table BuildTable made: rings and fades move on, a fade that produced its last sample ends, a
		// stream that has faded to none retires
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				r.start = false;
				r.pos = (unsigned)(((unsigned long long)r.pos + n) & (unsigned long long)(ringSamples - 1));
				r.hist = (int)std::min<unsigned long long>((unsigned long long)maxDelaySamples, (unsigned long long)r.hist + n);
				if (!r.fading) continue;
				r.k = (int)std::min<unsigned long long>((unsigned long long)r.N, (unsigned long long)r.k + n);
				if (r.k < r.N) continue;
				r.fading = false;
				r.N = r.k = 0;
				r.A = r.B;
				if (r.toNone) Retire(r);
			}
		}

	private:
		struct Row
		{
			bool has = false, fading = false, toNone = false, start = false;
			DelayParams A, B; // the setting it fades from, the one it has (fades to); equal outside a fade
			int N = 0, k = 0;
			unsigned pos = 0;
			int hist = 0;
		};
		// "no delay" as one end of a fade: the other end with wet = 0, dry = 1
		static DelayParams Silent(DelayParams p)
		{
			p.wet = 0.0f;
			p.dry = 1.0f;
			return p;
		}
		void Retire(Row& r)
		{
			r = Row();
			numEntries--;
		}
		std::vector<Row> rows;
		int maxDelaySamples = 0, ringSamples = 0, numEntries = 0;
	};

	// (delay_stage_kernels.hip) the launch of one piece over `count` entries of the device table: `n` samples of every entry's row from
	// sample `done` of the call on, rows `stride` floats apart, in place; rings `ringSamples` floats apart (a power of two), filter
	// states two floats a row
	struct DelayLaunch
	{
		const DelayEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long done;
		int n;
		float* rings;
		int ringSamples;
		DelayFilter* state;
	};

	unsigned long long DelayStageLaunches(); // launches of the stage's kernel so far (NA_DebugDelayLaunches)
}
