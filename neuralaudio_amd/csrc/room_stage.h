// room_stage.h -- the per-stream room stage of a batch: an algorithmic reverb -- a feedback delay network of eight
// lines, a two-tap damping FIR in front of an 8-point Hadamard mix -- on the row of every stream that has one, behind the delay stage
// and in front of the (convolution) reverb stage (NA_BatchEnableRoomStage / NA_BatchSetStreamRoom).  No reference counterpart: a host
// of the reference runs its reverb on the buffer it holds; here the rows stay on the device.
//
// This header is the host bookkeeping, the table units the kernel reads (room_stage_kernels.hip) and the ONE step function both sides
// run.  It uses no HIP, so that it compiles and runs on its own.  All of it is index arithmetic on arrays sized on the set-up side
// (Configure, Resize): the real-time calls -- Set, Leave, BuildTable, Advance -- allocate nothing.
//
// What is new against the delay stage (delay_stage.h): every line is at least kRoomPieceSamples long and the damping is a FIR, so no
// sample of a piece of kRoomPieceSamples samples reads what the piece writes -- the kernel runs lanes along the samples, and the mix of
// the eight lines is arithmetic inside one thread.  The lines live in eight rings per row on the device.  The host mirror counts
// positions: where the next sample goes in the rings (pos), how many samples the lines hold (hist, saturating at ringSamples) -- a read
// in front of T0 yields +0 by comparing positions, never by what a ring holds, so nothing is cleared on the device -- and where a fade
// stands (k).
//
// Arithmetic (the contract of include/neuralaudio_amd.h): every floating-point operation is one separately rounded f32 operation fl(.),
// round to nearest even, no FMA contraction (RoomStep below, compiled with contraction off), subnormals kept; integers exact.
// Constants of a setting: len_i = lineSamples[i], fb_i = feedback[i] (i = 0 .. 7), damp, wet, dry.  L_i[t] is what line i took at
// position t, counted from T0, the first sample after the set call that took the stream from no room; L_i[t] = +0 for t < 0.
// Per sample, x the row's sample and y what replaces it:
//   x'   = isnan(x) ? 0 : clamp(x, +-1e18f)
//   r_i  = L_i[t - len_i],  q_i = L_i[t - len_i - 1]
//   keep = fl(1 - damp)
//   d_i  = fl(fl(r_i * keep) + fl(q_i * damp))
//   h    = H8 d, the unnormalised Hadamard butterfly: three passes over pairs (a, b) -> (fl(a + b), fl(a - b)), the partners 1, then 2,
//          then 4 indices apart (the 1 / sqrt 8 is inside fb)
//   L_i[t] = fl(x' + fl(fb_i * h_i))
//   s    = fl(fl(fl(d_0 - d_1) + fl(d_2 - d_3)) + fl(fl(d_4 - d_5) + fl(d_6 - d_7)))
//   y    = fl(fl(dry * x') + fl(wet * s))
// Fades: a set call moves from setting A to B over N = fadeSamples, k counts the samples since the set call, wk = OutStageWeightAt(N, k).
// fb_i, damp, wet and dry are B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk)).  A line whose length differs between A and B
// cross-fades its read head as the delay stage does: r_i is B's tap where wk == 1, else fl(fl(fl(1 - wk) * tap_A) + fl(wk * tap_B)),
// and q_i likewise.  "None" as A is B with wet = 0, dry = 1; "none" as B is A with wet = 0, dry = 1, and the entry retires with the
// sample at which the fade ends.
// Stability: fb_i <= fl(1 / sqrt 8) < 1 / sqrt 8, H8 / sqrt 8 is orthogonal and the FIR's gain is at most 1 for damp in [0, 0.5], so the
// energy the lines hold never grows without input.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "output_stage.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_ROOM_HD __host__ __device__ __forceinline__
#else
#define NA_ROOM_HD inline
#endif

namespace na
{
	constexpr int kRoomLines = 8;
	constexpr int kRoomMinLineSamples = 128;     // a line is at least a piece long
	constexpr int kRoomMinMaxLine = 256;         // maxLineSamples: a power of two in [256, 16384]
	constexpr int kRoomMaxLineSamples = 16384;
	constexpr int kRoomPieceSamples = 128;       // the samples one pass of the kernel produces: nothing it reads was written inside it
	constexpr int kRoomWindow = kRoomPieceSamples + 1; // the samples of a line a piece reads: r and q of its 128 samples
	constexpr float kRoomMaxFeedback = 0.35355338f; // fl(1 / sqrt 8), which lies below 1 / sqrt 8
	constexpr float kRoomMaxDamp = 0.5f;
	constexpr float kRoomMaxMix = 1e6f;          // |wet|, |dry|

	// the constants of a room as the caller gives them (NA_RoomParams, field for field)
	struct RoomParams
	{
		int lineSamples[kRoomLines] = { 128, 128, 128, 128, 128, 128, 128, 128 };
		float feedback[kRoomLines] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
		float damp = 0.0f, wet = 0.0f, dry = 1.0f;
	};
	static_assert(sizeof(RoomParams) == 76, "NA_RoomParams is nineteen words");

	// nullptr: fine; else the text of the first rule the constants break (it names the field).  The lengths are held against
	// `maxLineSamples`, the batch's or -- without a batch -- the largest a batch can have.
	inline const char* RoomParamsError(const RoomParams& p, int maxLineSamples)
	{
		static const char* const lineTexts[kRoomLines] = { "lineSamples[0] must lie in [128, maxLineSamples]", "lineSamples[1] must lie in [128, maxLineSamples]",
			"lineSamples[2] must lie in [128, maxLineSamples]", "lineSamples[3] must lie in [128, maxLineSamples]", "lineSamples[4] must lie in [128, maxLineSamples]",
			"lineSamples[5] must lie in [128, maxLineSamples]", "lineSamples[6] must lie in [128, maxLineSamples]", "lineSamples[7] must lie in [128, maxLineSamples]" };
		static const char* const fbTexts[kRoomLines] = { "feedback[0] must lie in [0, 1 / sqrt 8]", "feedback[1] must lie in [0, 1 / sqrt 8]", "feedback[2] must lie in [0, 1 / sqrt 8]",
			"feedback[3] must lie in [0, 1 / sqrt 8]", "feedback[4] must lie in [0, 1 / sqrt 8]", "feedback[5] must lie in [0, 1 / sqrt 8]", "feedback[6] must lie in [0, 1 / sqrt 8]",
			"feedback[7] must lie in [0, 1 / sqrt 8]" };
		for (int i = 0; i < kRoomLines; i++)
			if (p.lineSamples[i] < kRoomMinLineSamples || p.lineSamples[i] > maxLineSamples) return lineTexts[i];
		for (int i = 0; i < kRoomLines; i++)
			if (!(p.feedback[i] >= 0.0f) || !(p.feedback[i] <= kRoomMaxFeedback)) return fbTexts[i];
		if (!(p.damp >= 0.0f) || !(p.damp <= kRoomMaxDamp)) return "damp must lie in [0, 0.5]";
		if (!std::isfinite(p.wet) || std::fabs(p.wet) > kRoomMaxMix) return "wet must be finite and at most 1e6 in magnitude";
		if (!std::isfinite(p.dry) || std::fabs(p.dry) > kRoomMaxMix) return "dry must be finite and at most 1e6 in magnitude";
		return nullptr;
	}

	// the smallest prime that is not below v (v >= 2)
	inline int RoomPrimeFrom(int v)
	{
		for (;; v++)
		{
			bool prime = v >= 2;
			for (int f = 2; f * f <= v && prime; f++) prime = v % f != 0;
			if (prime) return v;
		}
	}

	// NA_RoomParamsFromSeconds: host arithmetic in double, each value rounded once.  Line i is the smallest prime not below
	// rate * sizeMs / 1000 * 2^(-i / 8), clamped to [128, 16384] (mutually prime lengths: the lines' echoes do not pile up);
	// feedback[i] = 10^(-3 * lineSamples[i] / (decaySeconds * rate)) / sqrt 8 -- a circulation of line i loses what brings the tail 60 dB
	// down in decaySeconds --; wet = 10^(wetDb / 20) with -inf -> 0, dry likewise.  nullptr: fine; else what is wrong.
	inline const char* RoomParamsFromSeconds(int sampleRate, double sizeMs, double decaySeconds, double damp, double wetDb, double dryDb, RoomParams& out)
	{
		if (sampleRate < 1) return "sampleRate must be >= 1";
		if (!std::isfinite(sizeMs) || sizeMs < 0.0) return "sizeMs must be finite and at least 0";
		if (!std::isfinite(decaySeconds) || !(decaySeconds > 0.0)) return "decaySeconds must be finite and above 0";
		if (!std::isfinite(damp)) return "damp must lie in [0, 0.5]";
		if (std::isnan(wetDb) || wetDb == INFINITY) return "wet must be finite and at most 1e6 in magnitude";
		if (std::isnan(dryDb) || dryDb == INFINITY) return "dry must be finite and at most 1e6 in magnitude";
		const double rate = (double)sampleRate;
		RoomParams p;
		for (int i = 0; i < kRoomLines; i++)
		{
			const double want = rate * sizeMs / 1000.0 * std::pow(2.0, -(double)i / 8.0);
			int len = kRoomMaxLineSamples;
			if (want <= (double)kRoomMaxLineSamples) len = std::min(kRoomMaxLineSamples, RoomPrimeFrom(std::max(2, (int)std::ceil(want))));
			p.lineSamples[i] = std::max(kRoomMinLineSamples, len);
			p.feedback[i] = (float)(std::pow(10.0, -3.0 * (double)p.lineSamples[i] / (decaySeconds * rate)) / std::sqrt(8.0));
		}
		p.damp = (float)damp;
		p.wet = wetDb == -INFINITY ? 0.0f : (float)std::pow(10.0, wetDb / 20.0);
		p.dry = dryDb == -INFINITY ? 0.0f : (float)std::pow(10.0, dryDb / 20.0);
		if (const char* why = RoomParamsError(p, kRoomMaxLineSamples)) return why;
		out = p;
		return nullptr;
	}

	// The two settings of a row's fade (equal outside one) as the kernel reads them.  It lives in a block per row on the device and
	// travels once per set call: behind the entries of the first table built after the call (RoomEntry::set), from where the launch
	// files it in the row's block.
	struct RoomSetting
	{
		int lenA[kRoomLines], lenB[kRoomLines];
		float fbA[kRoomLines], fbB[kRoomLines];
		float dampA, dampB, wetA, wetB, dryA, dryB;
		int pad[2];
	};

	// One unit of work of the stage's launch: a row and where the call begins.  32 bytes: a table is a run of 32-byte units, the entries
	// first, behind them the settings that travel with this table, kRoomSetUnits units each.
	struct RoomEntry
	{
		int row = -1;
		int N = 0, k = 0;            // the fade: its length and the samples produced since the set call (0, 0: none)
		int toNone = 0;              // a fade to none: the entry retires with the sample at which the fade ends, later ones are not touched
		unsigned pos = 0;            // where the call's first sample goes in the row's rings
		int hist = 0;                // samples the lines hold in front of the call (saturating at ringSamples: enough for any length)
		int set = -1;                // index of the setting that comes with this table; -1: the row's block has it
		int pad = 0;
	};
	static_assert(sizeof(RoomEntry) == 32, "a table is a run of 32-byte units");
	static_assert(sizeof(RoomSetting) % sizeof(RoomEntry) == 0, "a setting is a whole number of units");
	constexpr int kRoomSetUnits = (int)(sizeof(RoomSetting) / sizeof(RoomEntry));
	constexpr int kRoomRowUnits = 1 + kRoomSetUnits; // what a row can put into one table: its entry and its setting

	// a ramped value of a sample: B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk))
	NA_ROOM_HD float RoomRamp(float gA, float gB, float wk)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (wk == 1.0f) return gB;
		const float span = gB - gA;
		const float part = span * wk;
		return gA + part;
	}

	// x' of a sample
	NA_ROOM_HD float RoomInput(float x) { return (x != x) ? 0.0f : fminf(fmaxf(x, -1e18f), 1e18f); }

	// a tap of a sample: B's where wk == 1 or the heads agree, else fl(fl(fl(1 - wk) * tap_A) + fl(wk * tap_B))
	NA_ROOM_HD float RoomTap(bool blend, float wk, float tapA, float tapB)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (!blend || wk == 1.0f) return tapB;
		const float rest = 1.0f - wk;
		const float partA = rest * tapA;
		const float partB = wk * tapB;
		return partA + partB;
	}

	// one sample: the contract above, line by line.  wk: the fade's weight at this sample (1 outside a fade); tap(i, a, back) =
	// L_i[t - len - back] with len = g.lenA[i] (a) or g.lenB[i] (!a), +0 in front of T0 -- the A taps are read only where the lengths
	// differ and wk < 1.  Returns y; line[i] is what goes into line i.
	template <class Tap>
	NA_ROOM_HD float RoomStep(const RoomSetting& g, float wk, float x, const Tap& tap, float (&line)[kRoomLines])
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float xs = RoomInput(x);
		const float damp = RoomRamp(g.dampA, g.dampB, wk);
		const float keep = 1.0f - damp;
		float d[kRoomLines], h[kRoomLines];
#if defined(__clang__)
#pragma unroll
#endif
		for (int i = 0; i < kRoomLines; i++)
		{
			const bool blend = wk != 1.0f && g.lenA[i] != g.lenB[i];
			const float r = RoomTap(blend, wk, blend ? tap(i, true, 0) : 0.0f, tap(i, false, 0));
			const float q = RoomTap(blend, wk, blend ? tap(i, true, 1) : 0.0f, tap(i, false, 1));
			const float near = r * keep;
			const float far = q * damp;
			d[i] = near + far;
			h[i] = d[i];
		}
#if defined(__clang__)
#pragma unroll
#endif
		for (int span = 1; span < kRoomLines; span *= 2)
		{
#if defined(__clang__)
#pragma unroll
#endif
			for (int i = 0; i < kRoomLines; i++)
			{
				if (i & span) continue;
				const float a = h[i], b = h[i + span];
				h[i] = a + b;
				h[i + span] = a - b;
			}
		}
#if defined(__clang__)
#pragma unroll
#endif
		for (int i = 0; i < kRoomLines; i++)
		{
			const float fb = RoomRamp(g.fbA[i], g.fbB[i], wk);
			const float back = fb * h[i];
			line[i] = xs + back;
		}
		const float s01 = d[0] - d[1], s23 = d[2] - d[3], s45 = d[4] - d[5], s67 = d[6] - d[7];
		const float low = s01 + s23, high = s45 + s67;
		const float s = low + high;
		const float wet = RoomRamp(g.wetA, g.wetB, wk);
		const float dry = RoomRamp(g.dryA, g.dryB, wk);
		const float direct = dry * xs;
		const float room = wet * s;
		return direct + room;
	}

	class RoomBook
	{
	public:
		// ---- set-up side ----
		// the smallest power of two that holds the longest line, its far tap and a piece
		static int RingFor(int maxLine)
		{
			int ring = 1;
			while (ring < maxLine + kRoomWindow) ring *= 2;
			return ring;
		}
		void Configure(int maxLine)
		{
			maxLineSamples = maxLine;
			ringSamples = RingFor(maxLine);
		}
		void Resize(int rowCount)
		{
			if (rowCount > (int)rows.size()) rows.resize((size_t)rowCount);
		}
		int Rows() const { return (int)rows.size(); }
		int MaxLine() const { return maxLineSamples; }
		int RingSamples() const { return ringSamples; }

		// ---- real-time side ----
		bool HasEntries() const { return numEntries > 0; }
		int NumEntries() const { return numEntries; }
		// a room that is not fading to none
		bool HasRoom(int s) const { return rows[(size_t)s].has && !rows[(size_t)s].toNone; }
		bool IsEntry(int s) const { return rows[(size_t)s].has; }
		const RoomParams& Target(int s) const { return rows[(size_t)s].B; }
		bool Fading(int s) const { return rows[(size_t)s].fading; }
		int FadeRemaining(int s) const { return rows[(size_t)s].fading ? rows[(size_t)s].N - rows[(size_t)s].k : 0; }

		// s: in no fade; p: valid (RoomParamsError) or nullptr: no room; N >= 0
		void Set(int s, const RoomParams* p, int N)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				if (!p) return;
				// T0: the lines start with the next sample
				r = Row();
				r.has = true;
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
			r.dirty = true;
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
		// park / removal: no room at once, the history is dropped
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (r.has) Retire(r);
		}

		// the units of the next call: entries into table[0 .. NumEntries()), behind them the settings of the set calls since the last
		// call; returns the entries, `units` the units to upload
		int BuildTable(RoomEntry* table, int& units) const
		{
			units = 0;
			if (numEntries == 0) return 0;
			int count = 0, sets = 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				RoomEntry e;
				e.row = (int)s;
				e.N = r.fading ? r.N : 0;
				e.k = r.fading ? r.k : 0;
				e.toNone = r.toNone ? 1 : 0;
				e.pos = r.pos;
				e.hist = r.hist;
				e.set = r.dirty ? sets++ : -1;
				if (e.set >= 0)
				{
					RoomSetting g;
					for (int i = 0; i < kRoomLines; i++)
					{
						g.lenA[i] = r.A.lineSamples[i];
						g.lenB[i] = r.B.lineSamples[i];
						g.fbA[i] = r.A.feedback[i];
						g.fbB[i] = r.B.feedback[i];
					}
					g.dampA = r.A.damp;
					g.dampB = r.B.damp;
					g.wetA = r.A.wet;
					g.wetB = r.B.wet;
					g.dryA = r.A.dry;
					g.dryB = r.B.dry;
					g.pad[0] = g.pad[1] = 0;
					std::memcpy(static_cast<void*>(table + numEntries + e.set * kRoomSetUnits), &g, sizeof(g));
				}
				table[count++] = e;
			}
			units = count + sets * kRoomSetUnits;
			return count;
		}

		// `n` samples were produced with the table BuildTable made: the settings are on the device, rings and fades move on, a fade that
		// produced its last sample ends (the kernel reads B alone outside a fade: nothing travels), a stream that has faded to none retires
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				r.dirty = false;
				r.pos = (unsigned)(((unsigned long long)r.pos + n) & (unsigned long long)(ringSamples - 1));
				r.hist = (int)std::min<unsigned long long>((unsigned long long)ringSamples, (unsigned long long)r.hist + n);
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
			bool dirty = false; // the settings changed since the last call
			RoomParams A, B;    // the setting it fades from, the one it has (fades to); equal outside a fade
			int N = 0, k = 0;
			unsigned pos = 0;
			int hist = 0;
		};
		// "none" as one end of a fade: the other end with wet = 0, dry = 1
		static RoomParams Silent(RoomParams p)
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
		int maxLineSamples = 0, ringSamples = 0, numEntries = 0;
	};

	// (room_stage_kernels.hip) the launch of one call over `count` entries of the device table (the settings that travel with it lie
	// behind them): `n` samples of every entry's row, rows `stride` floats apart, in place; a row's rings are kRoomLines x ringSamples
	// floats (a power of two), its setting block one RoomSetting
	struct RoomLaunch
	{
		const RoomEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long n;
		float* rings;
		int ringSamples;
		RoomSetting* settings;
	};

	unsigned long long RoomStageLaunches(); // launches of the stage's kernel so far (NA_DebugRoomLaunches)
}
