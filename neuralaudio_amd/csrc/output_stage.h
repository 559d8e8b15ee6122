// output_stage.h -- the per-stream output stage of a batch: ramped output gains and the cross-fade that hands a session
// from a live stream to another one (NA_BatchSetStreamGain / NA_BatchHandover).  No reference counterpart: the reference leaves both to
// its host (GetRecommendedOutputDBAdjustment, NeuralModel.h:92-95), which has the output rows in its hands; here they stay on the device.
//
// This header is the host bookkeeping and the table entry the kernel reads (output_stage_kernels.hip).  It uses no HIP, so that it
// compiles and runs on its own.  All of it is index arithmetic on arrays sized on the set-up side (Resize): the real-time calls
// -- SetGain, BeginFade, EndFadeOf, BuildTable, Advance -- allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h), all f32, shared by both sides through OutStageGainAt / OutStageWeightAt:
//   gain of the k-th sample after a set call:   g_a + (g_b - g_a) * ((min(k, R-1) + 1) / R)    (evaluated as (g_a * (R-1-k) + g_b * (k+1)) / R; g_b itself from k = R-1 on)
//   fade weight of the k-th sample of a fade:   w = (min(k, N-1) + 1) / N
// k is an integer kept per ramp / fade and advanced by whole calls: a sample's value depends on its position only, never on how the
// signal was cut into calls.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_OUTSTAGE_HD __host__ __device__ __forceinline__
#else
#define NA_OUTSTAGE_HD inline
#endif

namespace na
{
	constexpr int kOutStageMaxRamp = 1 << 20; // ramp and fade lengths: k + 1 is then exact in f32

	struct OutStageRamp
	{
		float g0 = 1.0f, g1 = 1.0f; // from, to
		int R = 0;                  // length in samples
		int k = 0;                  // samples produced since the set call, saturating at R (nothing changes beyond)
	};

	// One unit of work of the stage's launch: a single row (rowB < 0: row A is scaled by ramp a) or a fade pair (row A = `from`, row B =
	// `to`: A is scaled by a, B becomes (1 - w) * a * yA + w * b * yB -- the same thread reads both raw rows before it writes either).
	struct OutStageEntry
	{
		int rowA = -1, rowB = -1;
		OutStageRamp a, b;
		int N = 0, fk = 0; // fade length, samples of it produced
	};

	NA_OUTSTAGE_HD float OutStageGainAt(const OutStageRamp& r, long long k)
	{
		if (k >= (long long)r.R - 1) return r.g1;
		// the contract's g_a + (g_b - g_a) * ((k + 1) / R) as the convex sum it is: gains are >= 0, so nothing cancels and a ramp towards
		// 0 keeps its relative accuracy in its last samples, where the first form is left with the ratio's rounding alone
		return fmaf(r.g1, (float)(k + 1), r.g0 * (float)((long long)r.R - 1 - k)) / (float)r.R;
	}
	NA_OUTSTAGE_HD float OutStageWeightAt(int N, long long k)
	{
		if (k >= (long long)N - 1) return 1.0f;
		return (float)(k + 1) / (float)N;
	}

	class OutputStageBook
	{
	public:
		// set-up side: tables for `rows` rows (existing rows keep what they have)
		void Resize(int rows)
		{
			if (rows <= (int)gains.size()) return;
			gains.resize((size_t)rows);
			fadeOf.resize((size_t)rows, -1);
			fades.resize((size_t)(rows / 2 + 1));
			finished.reserve((size_t)(rows / 2 + 1));
		}
		int Rows() const { return (int)gains.size(); }
		bool HasEntries() const { return numGainEntries + numFades > 0; }
		int NumEntries() const { return numGainEntries + numFades; } // an upper bound of what BuildTable writes (a fade's streams count once)

		float Target(int s) const { return gains[(size_t)s].g1; }
		// the gain of the last sample produced (what a new ramp starts from)
		float Reached(int s) const
		{
			const OutStageRamp& r = gains[(size_t)s];
			return r.k == 0 ? r.g0 : OutStageGainAt(r, (long long)r.k - 1);
		}
		void SetGain(int s, float gain, int rampSamples)
		{
			OutStageRamp& r = gains[(size_t)s];
			const bool was = IsEntry(r);
			r.g0 = rampSamples > 0 ? Reached(s) : gain;
			r.g1 = gain;
			r.R = rampSamples;
			r.k = 0;
			numGainEntries += (int)IsEntry(r) - (int)was;
		}
		void ResetGain(int s) { SetGain(s, 1.0f, 0); }

		int FadeOf(int s) const { return fadeOf[(size_t)s]; }
		int FadeRemaining(int s) const
		{
			const int f = fadeOf[(size_t)s];
			return f < 0 ? 0 : fades[(size_t)f].N - fades[(size_t)f].k;
		}
		// from, to: in no fade; N >= 1.  false: no free slot (cannot happen with the tables Resize makes: a stream is in one fade at most)
		bool BeginFade(int from, int to, int N)
		{
			for (size_t f = 0; f < fades.size(); f++)
			{
				if (fades[f].live) continue;
				fades[f] = Fade{ from, to, N, 0, true };
				fadeOf[(size_t)from] = fadeOf[(size_t)to] = (int)f;
				numFades++;
				return true;
			}
			return false;
		}
		// the fade `s` is part of ends now (park / removal of either side); returns the other stream, -1: `s` was in none
		int EndFadeOf(int s)
		{
			const int f = fadeOf[(size_t)s];
			if (f < 0) return -1;
			Fade& fd = fades[(size_t)f];
			const int other = fd.from == s ? fd.to : fd.from;
			Release(f);
			return other;
		}

		// the entries of the next call, into table[0 .. NumEntries()); returns how many
		int BuildTable(OutStageEntry* table) const
		{
			int count = 0;
			if (numFades > 0)
				for (const Fade& fd : fades)
				{
					if (!fd.live) continue;
					OutStageEntry& e = table[count++];
					e.rowA = fd.from;
					e.rowB = fd.to;
					e.a = gains[(size_t)fd.from];
					e.b = gains[(size_t)fd.to];
					e.N = fd.N;
					e.fk = fd.k;
				}
			if (numGainEntries > 0)
				for (size_t s = 0; s < gains.size(); s++)
				{
					if (fadeOf[s] >= 0 || !IsEntry(gains[s])) continue;
					OutStageEntry& e = table[count++];
					e.rowA = (int)s;
					e.rowB = -1;
					e.a = gains[s];
					e.b = OutStageRamp();
					e.N = 0;
					e.fk = 0;
				}
			return count;
		}

		// `n` samples were produced with the table BuildTable made: ramps and fades move on, finished ramps at gain 1 retire, fades that
		// produced their last sample end -- their `from` streams wait in Finished() for the batch to park them
		void Advance(size_t n)
		{
			if (numGainEntries > 0)
				for (OutStageRamp& r : gains)
				{
					if (r.k >= r.R) continue;
					const bool was = IsEntry(r);
					r.k = (int)std::min<unsigned long long>((unsigned long long)r.R, (unsigned long long)r.k + n);
					if (r.k >= r.R) r.g0 = r.g1; // (a finished ramp is its target)
					numGainEntries += (int)IsEntry(r) - (int)was;
				}
			if (numFades > 0)
				for (size_t f = 0; f < fades.size(); f++)
				{
					Fade& fd = fades[f];
					if (!fd.live) continue;
					fd.k = (int)std::min<unsigned long long>((unsigned long long)fd.N, (unsigned long long)fd.k + n);
					if (fd.k < fd.N) continue;
					finished.push_back(fd.from);
					Release((int)f);
				}
		}
		std::vector<int>& Finished() { return finished; }

	private:
		struct Fade
		{
			int from = -1, to = -1, N = 0, k = 0;
			bool live = false;
		};
		static bool IsEntry(const OutStageRamp& r) { return r.g1 != 1.0f || r.k < r.R; }
		void Release(int f)
		{
			Fade& fd = fades[(size_t)f];
			fadeOf[(size_t)fd.from] = fadeOf[(size_t)fd.to] = -1;
			fd.live = false;
			numFades--;
		}
		std::vector<OutStageRamp> gains; // per row
		std::vector<int> fadeOf;         // per row: index into fades, -1
		std::vector<Fade> fades;
		std::vector<int> finished;
		int numGainEntries = 0, numFades = 0;
	};

	// (output_stage_kernels.hip) one launch over `count` entries of the device table: rows of `n` samples, `stride` floats apart, in place
	struct OutStageLaunch
	{
		const OutStageEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long n;
	};
}
