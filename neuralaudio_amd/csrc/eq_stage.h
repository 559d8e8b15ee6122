// eq_stage.h -- the per-stream EQ stage of a batch: a cascade of up to 8 biquad sections per stream -- the tone stack
// between the amp and the cabinet -- applied to the row the models produced, behind the gate's apply and in front of the cabinet stage
// (NA_BatchEnableEqStage / NA_BatchSetStreamEq).  No reference counterpart: a host of the reference runs its biquads on the buffer it
// holds; here the rows stay on the device.
//
// This header is the parameter check, the design function, the host bookkeeping, the table entry the kernel reads
// (eq_stage_kernels.hip) and the ONE step function both sides run.  It uses no HIP, so that it compiles and runs on its own.  The
// book is index arithmetic on arrays sized on the set-up side (Resize): the real-time calls -- Set, Leave, BuildTable, Advance --
// allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h): every operation is one separately rounded IEEE operation, no FMA contraction
// (EqSectionStep and EqMix below, compiled with contraction off); f64 and f32 subnormals are kept.  Per sample, x the row's sample:
//   x' = isnan(x) ? 0 : clamp(x, +-1e18f);  v = (double)x'
//   for sections 0 .. S-1 in order, each with its own x1, x2, y1, y2 (direct form I):
//     acc = fl(b0*v); acc = fl(acc + fl(b1*x1)); acc = fl(acc + fl(b2*x2));
//     acc = fl(acc - fl(a1*y1)); acc = fl(acc - fl(a2*y2));
//     x2 = x1; x1 = v; y2 = y1; y1 = acc; v = acc
//   o = (float)v
// k-th sample after a set call from cascade A to cascade B of length N: fl32(fl32(fl32(1 - w) * o_A) + fl32(w * o_B)) with
// w = OutStageWeightAt(N, k); o_B itself where w == 1.
//
// On the device a row has TWO slots, each a coefficient set and the states of 8 sections.  The cascade the row has (fades to) lives in
// slot `cur`, the one it fades from in the other.  A set call with N = 0 replaces the coefficients of slot `cur` and keeps its states;
// one with N > 0 fills the other slot, whose states start as copies of slot `cur`'s, and turns `cur` over.  Coefficients go up once:
// behind the entries of the first call after the set call, and the kernel files them into the row's slot.  What an entry says about
// states is where a slot's states are READ at the start of the call (`srcTo`) and how many leading sections of them stand (`keep*`:
// the others start at zero); they are always written to the slot itself.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "output_stage.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_EQ_HD __host__ __device__ __forceinline__
#else
#define NA_EQ_HD inline
#endif

namespace na
{
	constexpr int kEqMaxSections = 8;
	enum : int { kEqLowPass = 0, kEqHighPass = 1, kEqLowShelf = 2, kEqHighShelf = 3, kEqPeaking = 4 };

	// one biquad, normalised (a0 == 1): NA_EqSection
	struct EqSection
	{
		double b0 = 1.0, b1 = 0.0, b2 = 0.0, a1 = 0.0, a2 = 0.0;
	};
	// the history of one section (direct form I): 32 bytes, on the device per row, slot and section
	struct EqSecState
	{
		double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0;
	};
	// the coefficients of one cascade as they travel and as a slot keeps them
	struct EqCoefSet
	{
		EqSection s[kEqMaxSections];
	};

	// nullptr: fine; else the rule the section breaks
	inline const char* EqSectionError(const EqSection& c)
	{
		if (!std::isfinite(c.b0) || !std::isfinite(c.b1) || !std::isfinite(c.b2) || !std::isfinite(c.a1) || !std::isfinite(c.a2)) return "every coefficient must be finite";
		if (!(std::fabs(c.a2) < 1.0) || !(std::fabs(c.a1) < 1.0 + c.a2)) return "must be stable (|a2| < 1 and |a1| < 1 + a2)";
		return nullptr;
	}
	// "": fine; else the text of the first rule the cascade breaks (it names the section)
	inline std::string EqSectionsError(const EqSection* sections, int numSections)
	{
		if (numSections < 0 || numSections > kEqMaxSections) return "numSections must lie in [0, 8]";
		if (numSections > 0 && !sections) return "numSections must lie in [0, 8] (no sections given)";
		for (int i = 0; i < numSections; i++)
			if (const char* why = EqSectionError(sections[i])) return "section " + std::to_string(i) + ": " + why;
		return std::string();
	}

	// NA_EqSectionFromDesign: the RBJ cookbook in double, Q form: w0 = 2 pi f / Fs, alpha = sin(w0) / (2 Q), A = 10^(dB / 40), divided
	// through by a0.  nullptr: fine; else what is wrong.
	inline const char* EqSectionFromDesign(int kind, double sampleRate, double freqHz, double q, double gainDb, EqSection& out)
	{
		if (kind < kEqLowPass || kind > kEqPeaking) return "unknown kind (0 low-pass, 1 high-pass, 2 low shelf, 3 high shelf, 4 peaking)";
		if (!std::isfinite(sampleRate) || !std::isfinite(freqHz) || !std::isfinite(q) || !std::isfinite(gainDb)) return "every argument must be finite";
		if (!(sampleRate > 0.0)) return "sampleRate must be > 0";
		if (!(freqHz > 0.0) || !(freqHz < sampleRate / 2.0)) return "freqHz must lie in (0, sampleRate / 2)";
		if (!(q > 0.0)) return "q must be > 0";
		const double w0 = 2.0 * 3.14159265358979323846 * freqHz / sampleRate;
		const double cw = std::cos(w0), sw = std::sin(w0);
		const double alpha = sw / (2.0 * q);
		const double A = std::pow(10.0, gainDb / 40.0);
		double b0, b1, b2, a0, a1, a2;
		if (kind == kEqLowPass || kind == kEqHighPass)
		{
			const double s = kind == kEqLowPass ? 1.0 - cw : 1.0 + cw;
			b0 = s / 2.0;
			b1 = kind == kEqLowPass ? s : -s;
			b2 = s / 2.0;
			a0 = 1.0 + alpha;
			a1 = -2.0 * cw;
			a2 = 1.0 - alpha;
		}
		else if (kind == kEqPeaking)
		{
			b0 = 1.0 + alpha * A;
			b1 = -2.0 * cw;
			b2 = 1.0 - alpha * A;
			a0 = 1.0 + alpha / A;
			a1 = -2.0 * cw;
			a2 = 1.0 - alpha / A;
		}
		else
		{
			const double sq = 2.0 * std::sqrt(A) * alpha;
			const double sign = kind == kEqLowShelf ? 1.0 : -1.0; // (the high shelf is the low shelf with cos(w0) negated)
			const double c = sign * cw;
			b0 = A * ((A + 1.0) - (A - 1.0) * c + sq);
			b1 = sign * 2.0 * A * ((A - 1.0) - (A + 1.0) * c);
			b2 = A * ((A + 1.0) - (A - 1.0) * c - sq);
			a0 = (A + 1.0) + (A - 1.0) * c + sq;
			a1 = sign * -2.0 * ((A - 1.0) + (A + 1.0) * c);
			a2 = (A + 1.0) + (A - 1.0) * c - sq;
		}
		EqSection s;
		s.b0 = b0 / a0;
		s.b1 = b1 / a0;
		s.b2 = b2 / a0;
		s.a1 = a1 / a0;
		s.a2 = a2 / a0;
		if (const char* why = EqSectionError(s)) return why;
		out = s;
		return nullptr;
	}

	// the input sample as the cascade reads it: x' = isnan(x) ? 0 : clamp(x, +-1e18f)
	NA_EQ_HD float EqSanitize(float x) { return (x != x) ? 0.0f : fminf(fmaxf(x, -1e18f), 1e18f); }

	// one section, one sample: the contract above, line by line; returns acc
	NA_EQ_HD double EqSectionStep(const EqSection& c, EqSecState& s, double v)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		double acc = c.b0 * v;
		const double p1 = c.b1 * s.x1;
		acc = acc + p1;
		const double p2 = c.b2 * s.x2;
		acc = acc + p2;
		const double q1 = c.a1 * s.y1;
		acc = acc - q1;
		const double q2 = c.a2 * s.y2;
		acc = acc - q2;
		s.x2 = s.x1;
		s.x1 = v;
		s.y2 = s.y1;
		s.y1 = acc;
		return acc;
	}

	// the k-th sample of a fade of length N: fl32(fl32(fl32(1 - w) * o_A) + fl32(w * o_B)), o_B itself where w == 1
	NA_EQ_HD float EqMix(int N, long long k, float oA, float oB)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float w = OutStageWeightAt(N, k);
		if (w == 1.0f) return oB;
		const float u = 1.0f - w;
		const float a = u * oA;
		const float b = w * oB;
		return a + b;
	}

	// One unit of work of the stage's launch: a row, the slot of the cascade it has (fades to) and -- during a fade -- the cascade in the
	// other slot it fades from.  64 bytes: a coefficient set behind the entries of a table takes the room of kEqSetEntries entries.
	struct EqEntry
	{
		int row = -1;
		int slotTo = 0;            // `from` is the other slot
		int fading = 0;
		int STo = 0, SFrom = 0;    // sections of the two cascades; 0: the identity
		int N = 0, fk = 0;         // fade length, samples of it produced
		int srcTo = 0;             // the slot whose stored states `to` starts from ...
		int keepTo = 0;            // ... sections [0, keepTo) of them; the others start at zero
		int keepFrom = 0;          // sections of `from`'s own stored states that stand
		int coefTo = -1, coefFrom = -1; // index of the coefficient set that comes with this table; -1: the slot has its coefficients
		int pad[4] = { 0, 0, 0, 0 };
	};
	static_assert(sizeof(EqEntry) == 64, "a table is a run of 64-byte units");
	static_assert(sizeof(EqCoefSet) % sizeof(EqEntry) == 0, "a coefficient set is a whole number of units");
	constexpr int kEqSetEntries = (int)(sizeof(EqCoefSet) / sizeof(EqEntry));
	constexpr int kEqRowEntries = 1 + 2 * kEqSetEntries; // what a row can put into one table: its entry and the sets of both slots

	class EqBook
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
		bool Fading(int s) const { return rows[(size_t)s].has && rows[(size_t)s].fading; }
		int FadeRemaining(int s) const { return Fading(s) ? rows[(size_t)s].N - rows[(size_t)s].k : 0; }
		// the target cascade: its sections into out[0 .. min(count, capacity)); returns count
		int Target(int s, EqSection* out, int capacity) const
		{
			const Row& r = rows[(size_t)s];
			if (!r.has) return 0;
			const int S = r.S[r.cur];
			for (int i = 0; i < std::min(S, capacity); i++) out[i] = r.c[r.cur].s[i];
			return S;
		}

		// sections: valid (EqSectionsError); s: in no fade; N >= 0.  The stream runs cascade A (flat, with an all-zero history, if it has
		// no entry): B starts from A's states -- sections [0, min(S_A, S_B)) -- at the next sample, faded in over N samples.
		void Set(int s, const EqSection* sections, int S, int N)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				if (S == 0) return; // flat to flat
				r = Row();
				r.has = true;
				numEntries++;
			}
			const int a = r.cur;
			if (N == 0)
			{
				// the classic coefficient change on kept states: slot `cur` gets B's coefficients
				if (S == 0)
				{
					Retire(r);
					return;
				}
				Fill(r, a, sections, S);
				r.keep[a] = std::min(r.keep[a], S);
				return;
			}
			const int b = 1 - a;
			Fill(r, b, sections, S);
			r.src[b] = r.src[a]; // (== a: a set call during a fade is refused, and Advance has ended every other copy)
			r.keep[b] = std::min(r.keep[a], S);
			r.cur = b;
			r.fading = true;
			r.N = N;
			r.k = 0;
		}
		// park / removal: flat at once, the states are dropped
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (r.has) Retire(r);
		}

		// the units of the next call: entries into table[0 .. NumEntries()), behind them the coefficient sets of the set calls since the
		// last call; returns the entries, `units` the units to upload
		int BuildTable(EqEntry* table, int& units) const
		{
			units = 0;
			if (numEntries == 0) return 0;
			int count = 0, sets = 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				const int to = r.cur, from = 1 - r.cur;
				EqEntry e;
				e.row = (int)s;
				e.slotTo = to;
				e.fading = r.fading ? 1 : 0;
				e.STo = r.S[to];
				e.SFrom = r.fading ? r.S[from] : 0;
				e.N = r.N;
				e.fk = r.k;
				e.srcTo = r.src[to];
				e.keepTo = r.keep[to];
				e.keepFrom = r.fading ? r.keep[from] : 0;
				e.coefTo = (r.dirty[to] && r.S[to] > 0) ? sets++ : -1;
				e.coefFrom = (r.fading && r.dirty[from] && r.S[from] > 0) ? sets++ : -1;
				if (e.coefTo >= 0) std::memcpy(static_cast<void*>(table + numEntries + e.coefTo * kEqSetEntries), &r.c[to], sizeof(EqCoefSet));
				if (e.coefFrom >= 0) std::memcpy(static_cast<void*>(table + numEntries + e.coefFrom * kEqSetEntries), &r.c[from], sizeof(EqCoefSet));
				table[count++] = e;
			}
			units = count + sets * kEqSetEntries;
			return count;
		}

		// `n` samples were produced with the table BuildTable made: the coefficients are on the device and every slot's states are its
		// own; fades move on, a fade that produced its last sample ends (A is dropped), a stream that has faded to flat retires
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				for (int slot = 0; slot < 2; slot++)
				{
					r.dirty[slot] = false;
					r.src[slot] = slot;
					r.keep[slot] = r.S[slot];
				}
				if (!r.fading) continue;
				r.k = (int)std::min<unsigned long long>((unsigned long long)r.N, (unsigned long long)r.k + n);
				if (r.k < r.N) continue;
				r.fading = false;
				r.S[1 - r.cur] = 0;
				r.keep[1 - r.cur] = 0;
				if (r.S[r.cur] == 0) Retire(r);
			}
		}

	private:
		struct Row
		{
			bool has = false, fading = false;
			int cur = 0;                        // the slot of the cascade the row has (fades to)
			int S[2] = { 0, 0 };                // sections of the slots' cascades
			int src[2] = { 0, 1 }, keep[2] = { 0, 0 };
			bool dirty[2] = { false, false };   // the slot's coefficients changed since the last call
			int N = 0, k = 0;
			EqCoefSet c[2];
		};
		static void Fill(Row& r, int slot, const EqSection* sections, int S)
		{
			for (int i = 0; i < S; i++) r.c[slot].s[i] = sections[i];
			r.S[slot] = S;
			r.dirty[slot] = true;
		}
		void Retire(Row& r)
		{
			r = Row();
			numEntries--;
		}
		std::vector<Row> rows;
		int numEntries = 0;
	};

	// (eq_stage_kernels.hip) the launch over `count` entries of the device table, the coefficient sets that came with it behind them:
	// `n` samples of every entry's row, rows `stride` floats apart, in place; coefs [rows][2] sets, state [rows][2][8] section states
	struct EqLaunch
	{
		const EqEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long n;
		EqCoefSet* coefs;
		EqSecState* state;
	};

	unsigned long long EqStageLaunches(); // launches of the stage's kernel so far (NA_DebugEqLaunches)
}
