// mix_stage.h -- the mix stage of a batch: per-session mix groups -- the rows of up to 8 members (a stream's row as the
// output stage left it, or the input row the caller passed for it) summed through a ramped gain matrix into the rows of the group's
// first D members (NA_BatchEnableMixStage / NA_BatchSetMixGroup).  Behind the output stage and in front of the meter's OUT tap.  No
// reference counterpart: a host of the reference has every output buffer in its hands and sums there; here the rows stay on the device.
//
// This header is the host bookkeeping, the table entry the kernels read (mix_stage_kernels.hip) and the step functions both sides run.
// It uses no HIP, so that it compiles and runs on its own.  The book is index arithmetic on arrays sized on the set-up side (Resize):
// the real-time calls -- Set, Clear, Leave, BuildTable, Advance -- allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h): every operation is one separately rounded f32 operation, no FMA contraction
// (the step functions below, compiled with contraction off); the one exception is the ramp weight, an f64 quotient rounded to f32.
//   A group has one ramp (R, k) and two matrices g0 (from), g1 (to).
//     The gain of cell (d, j) at the k-th sample after the set call is g1 for k >= R - 1.
//     Before that it is fl(g0 + fl(fl(g1 - g0) * w)), with w = (float)((double)(k + 1) / (double)R).
//   For output d at a sample, the sum runs over the members j in member order whose gain at that sample is not exactly 0:
//     acc = fl(g_dj * y_j) for the first such member
//     acc = fl(acc + fl(g_dj * y_j)) for each further one
//     if there is no such member, the output is +0.0f
// k is an integer kept per group and advanced by whole calls: a sample's value depends on its position only, never on how the signal
// was cut into calls.  A set call during a ramp starts from the gains of the last sample produced (Reached: the same function); a new
// group starts from the identity matrix.  Rows are not sanitised.
//
// On the device a group's two matrices live in a block indexed by the row of its first member, [rows][2][8][8] floats.  They go up
// once: behind the entries of the first call after the set call, and the kernel files them into the block.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_MIX_HD __host__ __device__ __forceinline__
#else
#define NA_MIX_HD inline
#endif

namespace na
{
	constexpr int kMixMaxMembers = 8;
	constexpr int kMixMatrixFloats = kMixMaxMembers * kMixMaxMembers;   // cell (d, j) at d * 8 + j, whatever M
	constexpr int kMixSetFloats = 2 * kMixMatrixFloats;                 // g0 then g1
	constexpr int kMixMinDrySamples = 2048;
	enum : int { kMixTapOut = 0, kMixTapDry = 1 };

	// the ramp weight of the k-th sample (k < R - 1): the f64 quotient, rounded once to f32
	NA_MIX_HD float MixWeightAt(int R, long long k) { return (float)((double)(k + 1) / (double)R); }

	// fl(g0 + fl(fl(g1 - g0) * w))
	NA_MIX_HD float MixGainOf(float g0, float g1, float w)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float d = g1 - g0;
		const float p = d * w;
		return g0 + p;
	}

	// the gain of one cell at the k-th sample after the set call
	NA_MIX_HD float MixGainAt(float g0, float g1, int R, long long k)
	{
		if (k >= (long long)R - 1) return g1;
		return MixGainOf(g0, g1, MixWeightAt(R, k));
	}

	// one member of one output's sum: skipped where its gain is exactly 0 (either sign)
	NA_MIX_HD void MixAccumulate(float& acc, bool& any, float g, float y)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (g == 0.0f) return;
		const float p = g * y;
		acc = any ? acc + p : p;
		any = true;
	}

	// One unit of work of the stage's launches: a group.  64 bytes: a gain set behind the entries of a table takes the room of
	// kMixSetEntries entries.
	struct MixEntry
	{
		int M = 0, D = 0;   // members, outputs (the rows of the first D members)
		int R = 0, k = 0;   // the ramp: length, samples of it produced (saturating at R)
		int row[kMixMaxMembers] = { -1, -1, -1, -1, -1, -1, -1, -1 };
		int dryMask = 0;    // bit j: member j is the DRY tap of its stream
		int gainSet = -1;   // index of the gain set that comes with this table; -1: the block has the group's matrices
		int pad[2] = { 0, 0 };
	};
	static_assert(sizeof(MixEntry) == 64, "a table is a run of 64-byte units");
	constexpr int kMixSetEntries = (int)(kMixSetFloats * sizeof(float) / sizeof(MixEntry));
	static_assert(kMixSetEntries * sizeof(MixEntry) == kMixSetFloats * sizeof(float), "a gain set is a whole number of units");
	constexpr int kMixRowEntries = 1 + kMixSetEntries; // what a group can put into one table: its entry and its gain set

	class MixBook
	{
	public:
		struct Group
		{
			bool live = false, dirty = false;
			int M = 0, D = 0, R = 0, k = 0;
			int row[kMixMaxMembers] = {};
			int tap[kMixMaxMembers] = {};
			float g0[kMixMatrixFloats] = {}, g1[kMixMatrixFloats] = {};
		};

		// set-up side: tables for `rows` rows (existing groups stay)
		void Resize(int rowCount)
		{
			if (rowCount <= (int)groups.size()) return;
			groups.resize((size_t)rowCount);
			groupOf.resize((size_t)rowCount, -1);
		}
		int Rows() const { return (int)groups.size(); }

		// ---- real-time side ----
		bool HasEntries() const { return numGroups > 0; }
		int NumGroups() const { return numGroups; }
		bool HasDry() const { return numDry > 0; }
		// the group that names stream s (the row of its first member), -1: none
		int GroupOf(int s) const { return groupOf[(size_t)s]; }
		const Group& At(int g) const { return groups[(size_t)g]; }
		int RampRemaining(int g) const { return groups[(size_t)g].R - groups[(size_t)g].k; }
		// the member list is exactly that of group g: same order, taps and D
		bool Matches(int g, const int* streams, const int* taps, int M, int D) const
		{
			const Group& grp = groups[(size_t)g];
			if (!grp.live || grp.M != M || grp.D != D) return false;
			for (int j = 0; j < M; j++)
				if (grp.row[j] != streams[j] || grp.tap[j] != (taps ? taps[j] : kMixTapOut)) return false;
			return true;
		}
		// the gain of cell (d, j) at the last sample produced (what a new ramp starts from)
		float Reached(int g, int d, int j) const
		{
			const Group& grp = groups[(size_t)g];
			const int c = d * kMixMaxMembers + j;
			return grp.k == 0 ? grp.g0[c] : MixGainAt(grp.g0[c], grp.g1[c], grp.R, (long long)grp.k - 1);
		}

		// valid arguments (mix_stage.cpp checks the rules); gains [D][M].  The list of an existing group: a gain change from the gains
		// reached.  Else every stream is in no group: a new group, from the identity.
		void Set(const int* streams, const int* taps, int M, int D, const float* gains, int R)
		{
			const int g = streams[0];
			Group& grp = groups[(size_t)g];
			const bool change = groupOf[(size_t)g] == g && Matches(g, streams, taps, M, D);
			float from[kMixMatrixFloats] = {};
			for (int d = 0; d < D; d++)
				for (int j = 0; j < M; j++) from[d * kMixMaxMembers + j] = change ? Reached(g, d, j) : (d == j ? 1.0f : 0.0f);
			if (!change)
			{
				grp = Group();
				grp.live = true;
				grp.M = M;
				grp.D = D;
				bool dry = false;
				for (int j = 0; j < M; j++)
				{
					grp.row[j] = streams[j];
					grp.tap[j] = taps ? taps[j] : kMixTapOut;
					dry = dry || grp.tap[j] == kMixTapDry;
					groupOf[(size_t)streams[j]] = g;
				}
				numGroups++;
				numDry += dry ? 1 : 0;
			}
			for (int c = 0; c < kMixMatrixFloats; c++) grp.g0[c] = grp.g1[c] = 0.0f;
			for (int d = 0; d < D; d++)
				for (int j = 0; j < M; j++)
				{
					const int c = d * kMixMaxMembers + j;
					grp.g1[c] = gains[d * M + j];
					grp.g0[c] = R > 0 ? from[c] : grp.g1[c];
				}
			grp.R = R;
			grp.k = 0;
			grp.dirty = true;
		}
		// the group goes at once
		void Clear(int g)
		{
			Group& grp = groups[(size_t)g];
			if (!grp.live) return;
			bool dry = false;
			for (int j = 0; j < grp.M; j++)
			{
				groupOf[(size_t)grp.row[j]] = -1;
				dry = dry || grp.tap[j] == kMixTapDry;
			}
			grp.live = false;
			numGroups--;
			numDry -= dry ? 1 : 0;
		}
		// park / removal: the group that names the stream goes at once
		void Leave(int s)
		{
			if (groupOf[(size_t)s] >= 0) Clear(groupOf[(size_t)s]);
		}

		// the units of the next call: entries into table[0 .. NumGroups()), behind them the gain sets of the set calls since the last
		// call; returns the entries, `units` the units to upload
		int BuildTable(MixEntry* table, int& units) const
		{
			units = 0;
			if (numGroups == 0) return 0;
			int count = 0, sets = 0;
			for (size_t g = 0; g < groups.size() && count < numGroups; g++)
			{
				const Group& grp = groups[g];
				if (!grp.live) continue;
				MixEntry e;
				e.M = grp.M;
				e.D = grp.D;
				e.R = grp.R;
				e.k = grp.k;
				for (int j = 0; j < grp.M; j++)
				{
					e.row[j] = grp.row[j];
					if (grp.tap[j] == kMixTapDry) e.dryMask |= 1 << j;
				}
				if (grp.dirty)
				{
					e.gainSet = sets++;
					float* set = reinterpret_cast<float*>(table + numGroups + e.gainSet * kMixSetEntries);
					std::memcpy(set, grp.g0, sizeof(grp.g0));
					std::memcpy(set + kMixMatrixFloats, grp.g1, sizeof(grp.g1));
				}
				table[count++] = e;
			}
			units = count + sets * kMixSetEntries;
			return count;
		}

		// `n` samples were produced with the table BuildTable made: the matrices are on the device, the ramps move on
		void Advance(size_t n)
		{
			if (numGroups == 0 || n == 0) return;
			int seen = 0;
			for (size_t g = 0; g < groups.size() && seen < numGroups; g++)
			{
				Group& grp = groups[g];
				if (!grp.live) continue;
				seen++;
				grp.dirty = false;
				grp.k = (int)std::min<unsigned long long>((unsigned long long)grp.R, (unsigned long long)grp.k + n);
			}
		}

	private:
		std::vector<Group> groups; // per row: the group whose first member the row is
		std::vector<int> groupOf;  // per row: the group that names it, -1
		int numGroups = 0, numDry = 0;
	};

	// (mix_stage_kernels.hip) the launches over `count` entries of the device table, the gain sets that came with it behind them: `n`
	// samples, rows `stride` floats apart, in place; gains [rows][2][8][8]; stash [rows][drySamples] (the input rows of DRY members)
	struct MixLaunch
	{
		const MixEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long n;
		float* gains;
		float* stash;
		long drySamples;
	};
	struct MixStashLaunch
	{
		const MixEntry* table;
		int count;
		const float* in;
		long inStride;
		unsigned long long n;
		float* stash;
		long drySamples;
	};

	unsigned long long MixStageLaunches(); // launches of MixStageKernel so far (NA_DebugMixLaunches)
	unsigned long long MixStashLaunches(); // ... of MixStashKernel (NA_DebugMixStashLaunches)
}
