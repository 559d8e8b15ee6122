// mod_stage.h -- the per-stream modulation stage of a batch: chorus, flanger, vibrato and tremolo -- up to four voices
// that read a short delay line at a fractional, LFO-swept delay, an optional feedback of the first voice into the line, a wet / dry
// mix and an amplitude modulation -- on the row of every stream that has one, behind the compressor stage and in front of the delay
// stage (NA_BatchEnableModStage / NA_BatchSetStreamMod).  No reference counterpart: a host of the reference modulates the buffer it
// holds; here the rows stay on the device.
//
// This header is the host bookkeeping, the table entry the kernel reads (mod_stage_kernels.hip) and the step functions both sides run.
// It uses no HIP, so that it compiles and runs on its own (tests/mod_cases.cpp).  All of it is index arithmetic on arrays sized on the
// set-up side (Configure, Resize): the real-time calls -- Set, Leave, BuildTable, Advance -- allocate nothing.
//
// What is new against the delay stage (delay_stage.h): the delay of a sample is fractional and moves, but it is a function of the
// sample's integer position alone -- the LFO is a 32-bit phase, phase0 + j * phaseInc, folded into a triangle -- so every read address
// of a call is known up front, and the kernel runs lanes along the samples.  The line w lives in a ring per row on the device.  The host
// mirror counts positions: where the next sample goes in the ring (pos), how many samples the line holds (hist, saturating at
// maxDelaySamples) -- a read in front of T0 yields +0 by comparing positions, never by what the ring holds, so nothing is cleared on
// the device --, the LFO's phase at the next sample (phase) and where a fade stands (k).
//
// Arithmetic (the contract of include/neuralaudio_amd.h): every floating-point operation is one separately rounded f32 operation fl(.),
// round to nearest even, no FMA contraction (the step functions are compiled with contraction off), subnormals kept; integers exact.
// Positions: t counts the samples since T0, the first sample after the set call that took the stream from no modulation; k counts the
// samples since the last set call.  w[t] = +0 for t < 0.
// Limits of a setting: baseSamples >= 2; depthSamples >= 0; fl(baseSamples + depthSamples) <= maxDelaySamples - 2; numVoices in [1, 4];
// |voiceGain| <= 4; |feedback| <= 0.95; wet, dry finite, |.| <= 1e6; tremoloDepth in [0, 1]; shape NA_MOD_TRIANGLE or NA_MOD_SINE.
// LFO, no transcendental and no accumulation:
//   u_v = phaseAtSet + (unsigned)(k * phaseInc) + voicePhase[v]                 (modulo 2^32: the low word of the 64-bit product)
//   h   = (u_v & 0x80000000) ? ~u_v : u_v
//   tri = fl((float)(h >> 7) * 2^-24)                                           (exact, in [0, 1))
//   s_v = tri (triangle);  s_v = min(fl(fl(tri * tri) * fl(3 - fl(2 * tri))), 1) ("sine": the smoothstep of the triangle)
//   phaseAtSet is 0 at T0; every set call advances it by the old (unsigned)(k * phaseInc): a new rate acts at once on a continuous phase
//   (the book keeps the sum, `phase`, and advances it by whole calls).
// Per sample, x the row's sample and y what replaces it:
//   x'    = isnan(x) ? 0 : clamp(x, +-1e18f)
//   per voice v < numVoices:
//     D   = fl(base + fl(depth * s_v));  Di = (int)D;  fr = fl(D - (float)Di)
//     a   = w[t - Di];  b = w[t - Di - 1]                                       (+0 in front of the line's start)
//     tap_v = fl(a + fl(fr * fl(b - a)))
//   m     = fl(g_0 * tap_0), then m = fl(m + fl(g_v * tap_v)) in voice order
//   w[t]  = (fb == 0) ? x' : clamp(fl(x' + fl(fb * tap_0)), +-1e30f)
//   y0    = (wet == 0) ? fl(dry * x') : fl(fl(dry * x') + fl(wet * m))
//   y     = (td == 0) ? y0 : fl(y0 * fl(1 - fl(td * s_0)))
// Fades: a set call moves from setting A to B over N = fadeSamples, wk = OutStageWeightAt(N, k).  base, depth, fb, wet, dry, td and
// the four voice gains are B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk)) -- the delay is fractional already, so a new delay
// time glides, there is no read-head cross-fade.  A voice absent from a setting has gain 0 in it.  numVoices, voicePhase and phaseInc
// are B's from k = 0 (a set call that changes voicePhase[v] of a voice whose gain in A is non-zero is refused).  If the shapes differ,
// s_v = fl(fl(fl(1 - wk) * sA_v) + fl(wk * sB_v)) while wk != 1.  "None" as A is B with wet = 0, dry = 1, td = 0, fb = 0; "none" as B
// is A with wet = 0, dry = 1, td = 0, and the entry retires with the sample at which the fade ends.
// The chunk rule: Di >= floor(base), so samples t .. t + C - 1 read nothing the chunk writes when C <= floor(min(base_A, base_B)) - 1
// (the - 1 absorbs the ramp's one-ulp undershoot, which is also why base >= 2).  With fb == 0 in both settings w = x' and a whole
// piece is one chunk.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "output_stage.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_MOD_HD __host__ __device__ __forceinline__
#else
#define NA_MOD_HD inline
#endif

namespace na
{
	constexpr int kModMinDelaySamples = 8;     // maxDelaySamples lies in [8, 4096]
	constexpr int kModMaxDelaySamples = 4096;
	constexpr int kModPieceSamples = 2048;     // the longest run one launch processes; longer calls run in pieces
	constexpr int kModMaxVoices = 4;
	constexpr int kModTriangle = 0, kModSine = 1; // NA_MOD_TRIANGLE, NA_MOD_SINE
	constexpr float kModMaxFeedback = 0.95f;   // |feedback|
	constexpr float kModMaxMix = 1e6f;         // |wet|, |dry|
	constexpr float kModMaxVoiceGain = 4.0f;   // |voiceGain|

	// the constants of a modulation as the caller gives them (NA_ModParams, field for field)
	struct ModParams
	{
		float baseSamples = 2.0f, depthSamples = 0.0f;
		unsigned phaseInc = 0;
		int shape = kModTriangle, numVoices = 1;
		unsigned voicePhase[kModMaxVoices] = { 0, 0, 0, 0 };
		float voiceGain[kModMaxVoices] = { 1.0f, 0.0f, 0.0f, 0.0f };
		float feedback = 0.0f, wet = 0.0f, dry = 1.0f, tremoloDepth = 0.0f;
	};
	static_assert(sizeof(ModParams) == 68, "NA_ModParams is seventeen words");

	// nullptr: fine; else the text of the first rule the constants break (it names the field).  The reach is held against
	// `maxDelaySamples`, the batch's or -- without a batch -- the largest a batch can have.
	inline const char* ModParamsError(const ModParams& p, int maxDelaySamples)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (!std::isfinite(p.baseSamples) || p.baseSamples < 2.0f) return "baseSamples must be finite and at least 2";
		if (!std::isfinite(p.depthSamples) || p.depthSamples < 0.0f) return "depthSamples must be finite and at least 0";
		const float reach = p.baseSamples + p.depthSamples;
		if (!(reach <= (float)(maxDelaySamples - 2))) return "baseSamples + depthSamples must be at most maxDelaySamples - 2";
		if (p.shape != kModTriangle && p.shape != kModSine) return "shape must be NA_MOD_TRIANGLE or NA_MOD_SINE";
		if (p.numVoices < 1 || p.numVoices > kModMaxVoices) return "numVoices must lie in [1, 4]";
		static const char* const gainTexts[kModMaxVoices] = { "voiceGain[0] must be finite and at most 4 in magnitude", "voiceGain[1] must be finite and at most 4 in magnitude",
			"voiceGain[2] must be finite and at most 4 in magnitude", "voiceGain[3] must be finite and at most 4 in magnitude" };
		for (int v = 0; v < kModMaxVoices; v++)
			if (!std::isfinite(p.voiceGain[v]) || std::fabs(p.voiceGain[v]) > kModMaxVoiceGain) return gainTexts[v];
		if (!std::isfinite(p.feedback) || std::fabs(p.feedback) > kModMaxFeedback) return "feedback must lie in [-0.95, 0.95]";
		if (!std::isfinite(p.wet) || std::fabs(p.wet) > kModMaxMix) return "wet must be finite and at most 1e6 in magnitude";
		if (!std::isfinite(p.dry) || std::fabs(p.dry) > kModMaxMix) return "dry must be finite and at most 1e6 in magnitude";
		if (!std::isfinite(p.tremoloDepth) || p.tremoloDepth < 0.0f || p.tremoloDepth > 1.0f) return "tremoloDepth must lie in [0, 1]";
		return nullptr;
	}

	// NA_ModParamsFromMs: host arithmetic in double, each value rounded once.  baseSamples and depthSamples are ms * rate / 1000;
	// phaseInc = round(rateHz / rate * 2^32); voicePhase[v] = floor(v * 2^32 / voices); voiceGain[v] = 1 / voices; wet = 10^(wetDb / 20)
	// with -inf -> 0, dry likewise.  nullptr: fine; else what is wrong.
	inline const char* ModParamsFromMs(int sampleRate, double baseMs, double depthMs, double rateHz, int shape, int voices, double feedback, double wetDb, double dryDb,
		double tremoloDepth, ModParams& out)
	{
		if (sampleRate < 1) return "sampleRate must be >= 1";
		if (!std::isfinite(baseMs)) return "baseSamples must be finite and at least 2";
		if (!std::isfinite(depthMs)) return "depthSamples must be finite and at least 0";
		const double rate = (double)sampleRate;
		if (!std::isfinite(rateHz) || rateHz < 0.0 || rateHz > rate / 2.0) return "rateHz must lie in [0, sampleRate / 2]";
		if (voices < 1 || voices > kModMaxVoices) return "numVoices must lie in [1, 4]";
		if (!std::isfinite(feedback)) return "feedback must lie in [-0.95, 0.95]";
		if (std::isnan(wetDb) || wetDb == INFINITY) return "wet must be finite and at most 1e6 in magnitude";
		if (std::isnan(dryDb) || dryDb == INFINITY) return "dry must be finite and at most 1e6 in magnitude";
		if (!std::isfinite(tremoloDepth)) return "tremoloDepth must lie in [0, 1]";
		ModParams p;
		p.baseSamples = (float)(baseMs * rate / 1000.0);
		p.depthSamples = (float)(depthMs * rate / 1000.0);
		p.phaseInc = (unsigned)(unsigned long long)std::floor(rateHz / rate * 4294967296.0 + 0.5);
		p.shape = shape;
		p.numVoices = voices;
		for (int v = 0; v < kModMaxVoices; v++)
		{
			p.voicePhase[v] = v < voices ? (unsigned)(unsigned long long)std::floor((double)v * 4294967296.0 / (double)voices) : 0u;
			p.voiceGain[v] = v < voices ? (float)(1.0 / (double)voices) : 0.0f;
		}
		p.feedback = (float)feedback;
		p.wet = wetDb == -INFINITY ? 0.0f : (float)std::pow(10.0, wetDb / 20.0);
		p.dry = dryDb == -INFINITY ? 0.0f : (float)std::pow(10.0, dryDb / 20.0);
		p.tremoloDepth = (float)tremoloDepth;
		if (const char* why = ModParamsError(p, kModMaxDelaySamples)) return why;
		out = p;
		return nullptr;
	}

	// the ten values of a setting that ramp during a fade
	struct ModSetting
	{
		float base = 2.0f, depth = 0.0f, fb = 0.0f, wet = 0.0f, dry = 1.0f, td = 0.0f;
		float gain[kModMaxVoices] = { 0.0f, 0.0f, 0.0f, 0.0f };
	};

	// One unit of work of the stage's launch: a row, the two settings of its fade (equal outside one) and where the call begins.
	struct ModEntry
	{
		int row = -1;
		int N = 0, k = 0;            // the fade: its length and the samples produced since the set call (0, 0: none)
		int toNone = 0;              // a fade to none: the entry retires with the sample at which the fade ends, later ones are not touched
		int shapeA = 0, shapeB = 0;
		int numVoices = 1;           // B's from k = 0, as phaseInc and voicePhase
		unsigned phase = 0;          // the LFO's phase at the call's first sample: phaseAtSet + (unsigned)(k * phaseInc)
		unsigned phaseInc = 0;
		unsigned voicePhase[kModMaxVoices] = { 0, 0, 0, 0 };
		ModSetting A, B;             // the setting it fades from, the one it has (fades to)
		unsigned pos = 0;            // where the call's first sample goes in the row's ring
		int hist = 0;                // samples the line holds in front of the call (saturating at maxDelaySamples: enough for any reach)
		int reach = 4;               // the history window a sample can read: ceil(max(base_A + depth_A, base_B + depth_B)) + 2 <= maxDelaySamples
		int chunk = 0;               // 0: fb == 0 in both settings, the piece is one chunk; else floor(min(base_A, base_B)) - 1 >= 1
	};
	static_assert(sizeof(ModEntry) == 148, "an entry is thirty-seven words");

	// a ramped value of a sample: B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk))
	NA_MOD_HD float ModRamp(float gA, float gB, float wk)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (wk == 1.0f) return gB;
		const float span = gB - gA;
		const float part = span * wk;
		return gA + part;
	}

	NA_MOD_HD float ModClamp(float v, float limit) { return fminf(fmaxf(v, -limit), limit); }

	// x' of a sample
	NA_MOD_HD float ModInput(float x) { return (x != x) ? 0.0f : ModClamp(x, 1e18f); }

	// the triangle of a phase: exact, in [0, 1)
	NA_MOD_HD float ModTri(unsigned u)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const unsigned h = (u & 0x80000000u) ? ~u : u;
		return (float)(h >> 7) * 5.9604644775390625e-8f;
	}

	// s of a shape at a triangle value, in [0, 1]
	NA_MOD_HD float ModShape(int shape, float tri)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (shape == kModTriangle) return tri;
		const float square = tri * tri;
		const float twice = 2.0f * tri;
		const float rest = 3.0f - twice;
		const float smooth = square * rest;
		return fminf(smooth, 1.0f);
	}

	// s_v of a sample: B's shape, blended with A's while a fade between two shapes runs
	NA_MOD_HD float ModLfo(const ModEntry& e, float wk, unsigned u)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float tri = ModTri(u);
		const float sB = ModShape(e.shapeB, tri);
		if (wk == 1.0f || e.shapeA == e.shapeB) return sB;
		const float sA = ModShape(e.shapeA, tri);
		const float rest = 1.0f - wk;
		const float partA = rest * sA;
		const float partB = wk * sB;
		return partA + partB;
	}

	// one sample: the contract above, line by line.  k: the samples since the set call (the fade's position); j: the sample's index in
	// the call (the phase's); line(d) = w[t - d] for d >= 1, +0 in front of the line's start.  Returns y; `w` is what goes into the line.
	template <class Line>
	NA_MOD_HD float ModStep(const ModEntry& e, long long k, unsigned long long j, float x, const Line& line, float& w)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float wk = OutStageWeightAt(e.N, k);
		const float xs = ModInput(x);
		const float base = ModRamp(e.A.base, e.B.base, wk);
		const float depth = ModRamp(e.A.depth, e.B.depth, wk);
		const float fb = ModRamp(e.A.fb, e.B.fb, wk);
		const float wet = ModRamp(e.A.wet, e.B.wet, wk);
		const float dry = ModRamp(e.A.dry, e.B.dry, wk);
		const float td = ModRamp(e.A.td, e.B.td, wk);
		const unsigned u = e.phase + (unsigned)(j * (unsigned long long)e.phaseInc);
		float m = 0.0f, tap0 = 0.0f, s0 = 0.0f;
		// (a constant trip count: unrolled, the entry's arrays are read at constant indices and the entry stays in registers)
#if defined(__clang__)
#pragma unroll
#endif
		for (int v = 0; v < kModMaxVoices; v++)
		{
			if (v >= e.numVoices) break;
			const float s = ModLfo(e, wk, u + e.voicePhase[v]);
			const float sweep = depth * s;
			const float D = base + sweep;
			const int Di = (int)D;
			const float fr = D - (float)Di;
			const float a = line(Di);
			const float b = line(Di + 1);
			const float slope = b - a;
			const float part = fr * slope;
			const float tap = a + part;
			const float g = ModRamp(e.A.gain[v], e.B.gain[v], wk);
			const float voice = g * tap;
			if (v == 0)
			{
				m = voice;
				tap0 = tap;
				s0 = s;
			}
			else m = m + voice;
		}
		if (fb == 0.0f) w = xs;
		else
		{
			const float back = fb * tap0;
			const float sum = xs + back;
			w = ModClamp(sum, 1e30f);
		}
		const float direct = dry * xs;
		float y = direct;
		if (wet != 0.0f)
		{
			const float effect = wet * m;
			y = direct + effect;
		}
		if (td == 0.0f) return y;
		const float dip = td * s0;
		const float level = 1.0f - dip;
		return y * level;
	}

	class ModBook
	{
	public:
		// ---- set-up side ----
		// the smallest power of two that holds the longest reach and a piece
		static int RingFor(int maxDelay)
		{
			int ring = 1;
			while (ring < maxDelay + kModPieceSamples) ring *= 2;
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
		// a modulation that is not fading to none
		bool HasMod(int s) const { return rows[(size_t)s].has && !rows[(size_t)s].toNone; }
		bool IsEntry(int s) const { return rows[(size_t)s].has; }
		const ModParams& Target(int s) const { return rows[(size_t)s].B; }
		bool Fading(int s) const { return rows[(size_t)s].fading; }
		int FadeRemaining(int s) const { return rows[(size_t)s].fading ? rows[(size_t)s].N - rows[(size_t)s].k : 0; }
		// -1: fine; else the first voice that sounds in the setting the stream has and whose voicePhase `p` would change
		int PhaseClash(int s, const ModParams& p) const
		{
			const Row& r = rows[(size_t)s];
			if (!r.has) return -1;
			for (int v = 0; v < std::min(r.B.numVoices, p.numVoices); v++)
				if (r.B.voiceGain[v] != 0.0f && r.B.voicePhase[v] != p.voicePhase[v]) return v;
			return -1;
		}

		// s: in no fade; p: valid (ModParamsError, PhaseClash) or nullptr: no modulation; N >= 0
		void Set(int s, const ModParams* p, int N)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				if (!p) return;
				// T0: the line and the phase start with the next sample
				r = Row();
				r.has = true;
				numEntries++;
				r.B = *p;
				r.A = FromNone(*p);
			}
			else
			{
				r.A = r.B;
				r.B = p ? *p : ToNone(r.A);
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
		// park / removal: no modulation at once, the history is dropped
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (r.has) Retire(r);
		}

		// the entries of the next call, into table[0 .. NumEntries()); returns how many
		int BuildTable(ModEntry* table) const
		{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
			int count = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				ModEntry& e = table[count++];
				e.row = (int)s;
				e.N = r.fading ? r.N : 0;
				e.k = r.fading ? r.k : 0;
				e.toNone = r.toNone ? 1 : 0;
				e.shapeA = r.A.shape;
				e.shapeB = r.B.shape;
				e.numVoices = r.B.numVoices;
				e.phase = r.phase;
				e.phaseInc = r.B.phaseInc;
				for (int v = 0; v < kModMaxVoices; v++) e.voicePhase[v] = r.B.voicePhase[v];
				e.A = SettingOf(r.A);
				e.B = SettingOf(r.B);
				e.pos = r.pos;
				e.hist = r.hist;
				const float reachA = r.A.baseSamples + r.A.depthSamples;
				const float reachB = r.B.baseSamples + r.B.depthSamples;
				e.reach = std::min(maxDelaySamples, (int)std::ceil(std::max(reachA, reachB)) + 2);
				const bool feedsBack = r.A.feedback != 0.0f || r.B.feedback != 0.0f;
				e.chunk = feedsBack ? std::max(1, (int)std::floor(std::min(r.A.baseSamples, r.B.baseSamples)) - 1) : 0;
			}
			return count;
		}

		// `n` samples were produced with the table BuildTable made: rings, phases and fades move on, a fade that produced its last sample
		// ends, a stream that has faded to none retires
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				r.pos = (unsigned)(((unsigned long long)r.pos + n) & (unsigned long long)(ringSamples - 1));
				r.hist = (int)std::min<unsigned long long>((unsigned long long)maxDelaySamples, (unsigned long long)r.hist + n);
				r.phase += (unsigned)((unsigned long long)n * (unsigned long long)r.B.phaseInc);
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
			bool has = false, fading = false, toNone = false;
			ModParams A, B; // the setting it fades from, the one it has (fades to); equal outside a fade
			int N = 0, k = 0;
			unsigned pos = 0, phase = 0;
			int hist = 0;
		};
		// "none" as the start of a fade: the other end with wet = 0, dry = 1, td = 0, fb = 0
		static ModParams FromNone(ModParams p)
		{
			p.wet = 0.0f;
			p.dry = 1.0f;
			p.tremoloDepth = 0.0f;
			p.feedback = 0.0f;
			return p;
		}
		// "none" as the end of a fade: the other end with wet = 0, dry = 1, td = 0
		static ModParams ToNone(ModParams p)
		{
			p.wet = 0.0f;
			p.dry = 1.0f;
			p.tremoloDepth = 0.0f;
			return p;
		}
		// (a voice absent from a setting has gain 0 in it)
		static ModSetting SettingOf(const ModParams& p)
		{
			ModSetting g;
			g.base = p.baseSamples;
			g.depth = p.depthSamples;
			g.fb = p.feedback;
			g.wet = p.wet;
			g.dry = p.dry;
			g.td = p.tremoloDepth;
			for (int v = 0; v < kModMaxVoices; v++) g.gain[v] = v < p.numVoices ? p.voiceGain[v] : 0.0f;
			return g;
		}
		void Retire(Row& r)
		{
			r = Row();
			numEntries--;
		}
		std::vector<Row> rows;
		int maxDelaySamples = 0, ringSamples = 0, numEntries = 0;
	};

	// (mod_stage_kernels.hip) the launch of one piece over `count` entries of the device table: `n` samples of every entry's row from
	// sample `done` of the call on, rows `stride` floats apart, in place; rings `ringSamples` floats apart (a power of two)
	struct ModLaunch
	{
		const ModEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long done;
		int n;
		float* rings;
		int ringSamples;
	};

	unsigned long long ModStageLaunches(); // launches of the stage's kernel so far (NA_DebugModLaunches)
}
