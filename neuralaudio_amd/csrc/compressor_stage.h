// compressor_stage.h -- the per-stream compressor stage of a batch: a feed-forward compressor (with an infinite ratio a
// limiter) on the row the models produced, behind the cabinet stage and in front of the delay stage -- dynamics in front of the
// time-based effects (NA_BatchEnableCompressorStage / NA_BatchSetStreamCompressor).  No reference counterpart: a host of the reference
// runs its dynamics on the buffer it holds; here the rows stay on the device.
//
// This header is the parameter check, the design function, the host bookkeeping, the table entry the kernel reads
// (compressor_stage_kernels.hip) and the step functions both sides run.  It uses no HIP, so that it compiles and runs on its own.  The
// book is index arithmetic on arrays sized on the set-up side (Resize): the real-time calls -- Set, Leave, BuildTable, Advance --
// allocate nothing.
//
// Topology: a branching peak follower runs on the row's own samples, a static gain curve is read at the follower's level, the row is
// multiplied.  The gain computer has no transcendental: a curve is a table of 513 gains on a level axis that is the float's own bit
// pattern -- 16 knots per octave from 2^-24 to 2^8, interpolated linearly.  Knot i sits at level 2^(-24 + (i >> 4)) * (1 + (i & 15) / 16).
//
// Arithmetic (the contract of include/neuralaudio_amd.h): every operation is one separately rounded f32 operation, no FMA contraction
// (CompFollow, CompCurveAt and CompGain below, compiled with contraction off); subnormals are kept.  Constants of an entry: aA, aR in
// (0, 1]; curve t[0..512], every value finite and in [0, 65536].  State per row: f32 e (starts at +0) and the last g.  Per sample, x
// the row's sample:
//   x' = (x is NaN) ? 0 : min(|x|, 255.0f)
//   c  = (x' > e) ? aA : aR
//   d  = fl(x' - e);  e = fl(e + fl(c * d))
//   b  = bits(e);  q = b >> 19
//   curve(t): q < 1648 ? t[0]
//             : i = min(q - 1648, 511);  f = fl((float)(b & 0x7FFFF) * 2^-19);
//               fl(t[i] + fl(f * fl(t[i+1] - t[i])))
//   g  = curve(tB)                                              where w == 1
//   g  = fl(fl(fl(1 - w) * curve(tA)) + fl(w * curve(tB)))      else, w = OutStageWeightAt(N, k)
//   y  = fl(x * g)
// e never leaves [0, 2^8), so i + 1 <= 512.  The argument: x' lies in [0, 255] and c in (0, 1].  Where x' > e: d = fl(x' - e) > 0 and
// fl(c * d) <= d (rounding is monotone and d is a float), so the new e is at most fl(e + d) <= fl(x' * (1 + 2^-24)) <= 255 + 2^-16; it
// is at least e.  Where x' <= e: d <= 0 and |fl(c * d)| <= |d| <= e (e >= x' >= 0, monotone rounding again), so the new e lies in
// [0, e], and an exact cancellation gives +0 in round-to-nearest: e is never -0.  So bits(e) < bits(256.0f) = 0x43800000 and
// q <= 2159 = 1648 + 511: the min in the curve's line is never taken.  A NaN or infinite sample goes through the multiplication as it
// is; the follower sees 0 or 255.
//
// A row has TWO curve slots on the device, as the EQ has two cascades: tB, the curve it has or fades to, lives in slot `cur`; tA, the
// one it fades from, in the other.  "No compressor" is the unity curve: g = 1, never read from memory (a slot's `unity` flag).  A set
// call with N = 0 replaces the curve of slot `cur`; one with N > 0 fills the other slot and turns `cur` over.  New aA / aR act from the
// next sample on the kept e: only curves fade.  Curves go up once: behind the entries of the first call after the set call, and the
// kernel files them into the row's slot.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "output_stage.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_COMP_HD __host__ __device__ __forceinline__
#else
#define NA_COMP_HD inline
#endif

namespace na
{
	constexpr int kCompCurvePoints = 513;     // knots of a curve: 32 octaves of 16 and the closing one
	constexpr int kCompCurveFloats = 528;     // ... as a curve travels and as a slot keeps it: 33 table units
	constexpr unsigned kCompFirstQ = 1648u;   // bits(2^-24) >> 19: the level of knot 0
	constexpr float kCompMaxLevel = 255.0f;   // what the follower sees at the most
	constexpr float kCompMaxGain = 65536.0f;  // ... and a curve holds at the most

	// the constants of a compressor as the caller gives them, field for field the public
	//   typedef struct NA_CompressorParams { float attackCoeff, releaseCoeff; float curve[513]; } NA_CompressorParams;
	// (what NA_BatchGetCompressorInfo fills is
	//   typedef struct NA_CompressorInfo { int curvePoints, numCompressors; long long deviceBytes; } NA_CompressorInfo;
	// from CompressorStageInfo, gpu_batch.h)
	struct CompParams
	{
		float attackCoeff = 1.0f, releaseCoeff = 1.0f;
		float curve[kCompCurvePoints];
	};

	// the level of knot i, exactly (a float: five significant bits)
	inline double CompKnotLevel(int i) { return std::ldexp(1.0 + (double)(i & 15) / 16.0, -24 + (i >> 4)); }

	// "": fine; else the text of the first rule the constants break (it names the field)
	inline std::string CompParamsError(const CompParams& p)
	{
		if (!std::isfinite(p.attackCoeff)) return "attackCoeff must be finite";
		if (!std::isfinite(p.releaseCoeff)) return "releaseCoeff must be finite";
		if (!(p.attackCoeff > 0.0f) || p.attackCoeff > 1.0f) return "attackCoeff must lie in (0, 1]";
		if (!(p.releaseCoeff > 0.0f) || p.releaseCoeff > 1.0f) return "releaseCoeff must lie in (0, 1]";
		for (int i = 0; i < kCompCurvePoints; i++)
		{
			if (!std::isfinite(p.curve[i])) return "curve[" + std::to_string(i) + "] must be finite";
			if (p.curve[i] < 0.0f || p.curve[i] > kCompMaxGain) return "curve[" + std::to_string(i) + "] must lie in [0, 65536]";
		}
		return std::string();
	}

	// NA_CompressorParamsFromDb: coefficients 1 - exp(-1 / (ms * rate / 1000)) in double, rounded once (the gate's formula; ms == 0 gives
	// 1).  Per knot, in double, with L = 20 log10(level_i), o = L - thresholdDb, s = 1 / ratio - 1 (ratio in [1, +inf], +inf gives
	// s = -1) and W = kneeDb >= 0:  G = 0 if 2o < -W;  G = s (o + W/2)^2 / (2W) if 2|o| <= W;  G = s o else;
	// t[i] = (float)10^((G + makeupDb) / 20).  (W = 0 leaves the middle line one point, o = 0, where both neighbours give 0.)
	// "": fine; else what is wrong.
	inline std::string CompParamsFromDb(int sampleRate, float thresholdDb, float ratio, float kneeDb, float makeupDb, float attackMs, float releaseMs, CompParams& out)
	{
		if (sampleRate < 1) return "sampleRate must be >= 1";
		if (!std::isfinite(thresholdDb)) return "thresholdDb must be finite";
		if (std::isnan(ratio) || ratio < 1.0f) return "ratio must lie in [1, +inf]";
		if (!std::isfinite(kneeDb) || kneeDb < 0.0f) return "kneeDb must be finite and >= 0";
		if (!std::isfinite(makeupDb)) return "makeupDb must be finite";
		if (!std::isfinite(attackMs) || attackMs < 0.0f) return "attackMs must be finite and >= 0";
		if (!std::isfinite(releaseMs) || releaseMs < 0.0f) return "releaseMs must be finite and >= 0";
		const double rate = (double)sampleRate;
		const auto coeff = [&](float ms) { return ms == 0.0f ? 1.0f : (float)(1.0 - std::exp(-1.0 / ((double)ms * rate / 1000.0))); };
		CompParams p;
		p.attackCoeff = coeff(attackMs);
		p.releaseCoeff = coeff(releaseMs);
		const double s = 1.0 / (double)ratio - 1.0, W = (double)kneeDb;
		for (int i = 0; i < kCompCurvePoints; i++)
		{
			const double L = 20.0 * std::log10(CompKnotLevel(i));
			const double o = L - (double)thresholdDb;
			double G;
			if (2.0 * o < -W) G = 0.0;
			else if (W > 0.0 && 2.0 * std::fabs(o) <= W) G = s * (o + W / 2.0) * (o + W / 2.0) / (2.0 * W);
			else G = s * o;
			p.curve[i] = (float)std::pow(10.0, (G + (double)makeupDb) / 20.0);
		}
		const std::string why = CompParamsError(p);
		if (!why.empty()) return why + " (thresholdDb, ratio, kneeDb and makeupDb give a gain outside the curve's range)";
		out = p;
		return std::string();
	}

	// per row, on the device (8 bytes)
	struct CompState
	{
		float e = 0.0f; // the follower
		float g = 1.0f; // the g of the last sample produced
	};

	// a curve as it travels and as a slot keeps it
	struct CompCurve
	{
		float t[kCompCurveFloats];
	};

	NA_COMP_HD uint32_t CompBits(float v)
	{
		return __builtin_bit_cast(uint32_t, v);
	}

	// x' of the contract
	NA_COMP_HD float CompLevel(float x) { return (x != x) ? 0.0f : fminf(fabsf(x), kCompMaxLevel); }

	// the follower's step on x' = CompLevel(x): the contract's second and third lines; returns the new e
	NA_COMP_HD float CompFollow(float aA, float aR, float e, float xa)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float c = (xa > e) ? aA : aR;
		const float d = xa - e;
		const float cd = c * d;
		return e + cd;
	}

	// curve(t) at the follower's level e
	NA_COMP_HD float CompCurveAt(const float* t, float e)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const uint32_t b = CompBits(e);
		const uint32_t q = b >> 19;
		if (q < kCompFirstQ) return t[0];
		const uint32_t i = (q - kCompFirstQ < 511u) ? q - kCompFirstQ : 511u;
		const float f = (float)(b & 0x7FFFFu) * 1.9073486328125e-06f; // 2^-19: exact scaling of a 19-bit integer
		const float lo = t[i];
		const float rise = t[i + 1] - lo;
		const float part = f * rise;
		return lo + part;
	}

	// g of the contract from the two curves' values: gB itself where w == 1
	NA_COMP_HD float CompGain(float w, float gA, float gB)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (w == 1.0f) return gB;
		const float u = 1.0f - w;
		const float a = u * gA;
		const float b = w * gB;
		return a + b;
	}

	// One unit of work of the stage's launch: a row, the slot of the curve it has (fades to) and -- during a fade -- the curve in the
	// other slot it fades from.  64 bytes: a curve behind the entries of a table takes the room of kCompCurveEntries entries.
	struct CompEntry
	{
		int row = -1;
		int slotTo = 0;             // `from` is the other slot
		int fading = 0;
		int N = 0, fk = 0;          // fade length, samples of it produced
		int start = 0;              // the call begins from e = +0 instead of the stored state (no memset travels with a set call)
		int unityTo = 0, unityFrom = 0; // the slot's curve is the unity curve: g = 1, nothing is read
		int coefTo = -1, coefFrom = -1; // index of the curve that comes with this table; -1: the slot has its curve
		float aA = 1.0f, aR = 1.0f;
		int pad[4] = { 0, 0, 0, 0 };
	};
	static_assert(sizeof(CompEntry) == 64, "a table is a run of 64-byte units");
	static_assert(sizeof(CompCurve) % sizeof(CompEntry) == 0, "a curve is a whole number of units");
	constexpr int kCompCurveEntries = (int)(sizeof(CompCurve) / sizeof(CompEntry));
	constexpr int kCompRowEntries = 1 + 2 * kCompCurveEntries; // what a row can put into one table: its entry and the curves of both slots

	class CompBook
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
		bool IsEntry(int s) const { return rows[(size_t)s].has; }
		// a compressor that is not fading to none
		bool HasCompressor(int s) const { return rows[(size_t)s].has && !rows[(size_t)s].unity[rows[(size_t)s].cur]; }
		bool Fading(int s) const { return rows[(size_t)s].has && rows[(size_t)s].fading; }
		int FadeRemaining(int s) const { return Fading(s) ? rows[(size_t)s].N - rows[(size_t)s].k : 0; }
		bool Starting(int s) const { return rows[(size_t)s].has && rows[(size_t)s].start; } // no sample produced since it came
		// the target: HasCompressor(s)
		void Target(int s, CompParams& out) const
		{
			const Row& r = rows[(size_t)s];
			out.attackCoeff = r.aA;
			out.releaseCoeff = r.aR;
			std::memcpy(out.curve, r.c[r.cur].t, sizeof(out.curve));
		}

		// p: valid (CompParamsError) or nullptr (none: the unity curve); s: in no fade; N >= 0.  A stream without an entry starts from
		// the unity curve with e = +0.  The target curve acts from the next sample, faded in over N samples; the coefficients switch at
		// once (nullptr keeps them: the follower goes on through the fade).
		void Set(int s, const CompParams* p, int N)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				if (!p) return; // none to none
				r.has = true;
				r.fading = false;
				r.cur = 0;
				r.unity[0] = r.unity[1] = true;
				r.dirty[0] = r.dirty[1] = false;
				r.N = r.k = 0;
				r.start = true;
				numEntries++;
			}
			if (p)
			{
				r.aA = p->attackCoeff;
				r.aR = p->releaseCoeff;
			}
			if (N == 0)
			{
				if (!p)
				{
					Retire(r);
					return;
				}
				Fill(r, r.cur, *p);
				return;
			}
			const int b = 1 - r.cur;
			if (p) Fill(r, b, *p);
			else
			{
				r.unity[b] = true;
				r.dirty[b] = false;
			}
			r.cur = b;
			r.fading = true;
			r.N = N;
			r.k = 0;
		}
		// park / removal: no compressor at once, the state is dropped
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (r.has) Retire(r);
		}

		// the units of the next call: entries into table[0 .. NumEntries()), behind them the curves of the set calls since the last
		// call; returns the entries, `units` the units to upload
		int BuildTable(CompEntry* table, int& units) const
		{
			units = 0;
			if (numEntries == 0) return 0;
			int count = 0, sets = 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				const int to = r.cur, from = 1 - r.cur;
				CompEntry e;
				e.row = (int)s;
				e.slotTo = to;
				e.fading = r.fading ? 1 : 0;
				e.N = r.N;
				e.fk = r.k;
				e.start = r.start ? 1 : 0;
				e.unityTo = r.unity[to] ? 1 : 0;
				e.unityFrom = (!r.fading || r.unity[from]) ? 1 : 0;
				e.coefTo = (r.dirty[to] && !r.unity[to]) ? sets++ : -1;
				e.coefFrom = (r.fading && r.dirty[from] && !r.unity[from]) ? sets++ : -1;
				e.aA = r.aA;
				e.aR = r.aR;
				if (e.coefTo >= 0) std::memcpy(static_cast<void*>(table + numEntries + e.coefTo * kCompCurveEntries), &r.c[to], sizeof(CompCurve));
				if (e.coefFrom >= 0) std::memcpy(static_cast<void*>(table + numEntries + e.coefFrom * kCompCurveEntries), &r.c[from], sizeof(CompCurve));
				table[count++] = e;
			}
			units = count + sets * kCompCurveEntries;
			return count;
		}

		// `n` samples were produced with the table BuildTable made: the curves are on the device and the state is the row's own; fades
		// move on, a fade that produced its last sample ends (tA is dropped), a stream that has faded to none retires
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				r.dirty[0] = r.dirty[1] = false;
				r.start = false;
				if (!r.fading) continue;
				r.k = (int)std::min<unsigned long long>((unsigned long long)r.N, (unsigned long long)r.k + n);
				if (r.k < r.N) continue;
				r.fading = false;
				r.unity[1 - r.cur] = true;
				if (r.unity[r.cur]) Retire(r);
			}
		}

	private:
		struct Row
		{
			bool has = false, fading = false, start = false;
			int cur = 0;                        // the slot of the curve the row has (fades to)
			bool unity[2] = { true, true };     // the slot holds the unity curve (nothing of c[slot] counts)
			bool dirty[2] = { false, false };   // the slot's curve changed since the last call
			int N = 0, k = 0;
			float aA = 1.0f, aR = 1.0f;
			CompCurve c[2];
		};
		static void Fill(Row& r, int slot, const CompParams& p)
		{
			std::memcpy(r.c[slot].t, p.curve, sizeof(p.curve));
			for (int i = kCompCurvePoints; i < kCompCurveFloats; i++) r.c[slot].t[i] = 0.0f;
			r.unity[slot] = false;
			r.dirty[slot] = true;
		}
		// (the curves' memory is left as it is: 4 KB that nothing reads again)
		void Retire(Row& r)
		{
			r.has = r.fading = r.start = false;
			r.unity[0] = r.unity[1] = true;
			r.dirty[0] = r.dirty[1] = false;
			r.N = r.k = 0;
			numEntries--;
		}
		std::vector<Row> rows;
		int numEntries = 0;
	};

	// (compressor_stage_kernels.hip) the launch over `count` entries of the device table, the curves that came with it behind them: `n`
	// samples of every entry's row, rows `stride` floats apart, in place; curves [rows][2], state [rows]
	struct CompLaunch
	{
		const CompEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long n;
		CompCurve* curves;
		CompState* state;
	};

	constexpr int kCompGroupEntries = 16; // entries of one workgroup of the launch

	unsigned long long CompressorStageLaunches(); // launches of the stage's kernel so far (NA_DebugCompressorLaunches)
}
