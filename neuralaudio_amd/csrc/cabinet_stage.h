// cabinet_stage.h -- the per-stream cabinet stage of a batch: every stream that has an impulse response (IR) gets its
// row replaced by the row's convolution with that IR, behind the model launches and in front of the output stage
// (NA_BatchEnableCabinetStage / NA_BatchLoadIR / NA_BatchSetStreamIR).  No reference counterpart: a host of the reference convolves the
// model output with its cabinet itself, because it has the samples in its hands; here they stay on the device.
//
// This header is the host bookkeeping and the table entry the kernels read (cabinet_stage_kernels.hip).  It uses no HIP, so that it
// compiles and runs on its own.  All of it is index arithmetic on arrays sized on the set-up side (Configure, Resize, AddIR): the
// real-time calls -- SetIR, BuildTable, Advance, Leave -- allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h), all f32; positions count the samples the caller sees:
//   c_h[t] = sum over k in [0, K) of h[k] * y[t - k],  y[t] = 0 for t < T0;  the dry path is the one-tap IR {1}: c_dry[t] = y[t]
//   k-th sample after a set call from A to B of length N:  (1 - w) * c_A[t] + w * c_B[t],  w = (min(k, N-1) + 1) / N  (OutStageWeightAt)
// Summation order of one output (CabSliceOf, cabinet_stage_kernels.hip): tap k belongs to slice (k / kCabSliceTaps) % kCabSlices; a
// slice is summed by FMAs in rising k from +0, the slices are added in rising slice number.  A function of k alone: nothing of the
// call, the row, the launch or maxTaps enters it.
//
// The ring of a row holds its raw samples (the model's output): ringSamples is a power of two >= maxTaps - 1 + pieceSamples, so a piece
// of a call is appended whole before the convolution reads the maxTaps - 1 samples in front of it.  `hist` counts the samples of the
// ring that belong to the stream's present history (since T0); what lies before them reads as zero, so that nothing has to be cleared
// when a stream's history is dropped.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "output_stage.h"

namespace na
{
	constexpr int kCabMaxTaps = 8192;
	constexpr int kCabPieceSamples = 2048; // the longest run the stage processes at once
	constexpr int kCabSlices = 8;          // partial sums per output ...
	constexpr int kCabSliceTaps = 128;     // ... each over runs of this many consecutive taps
	constexpr int kCabTileTaps = kCabSlices * kCabSliceTaps; // taps the kernel holds in LDS at a time
	constexpr int kCabBlockOutputs = 128;  // outputs of one workgroup
	constexpr int kCabDry = -1;            // the IR id of the dry path

	inline int CabSliceOf(int k) { return (k / kCabSliceTaps) % kCabSlices; }

	// One unit of work of the stage's launches: a row, its IR and -- during a fade -- the IR it fades from.  taps == nullptr: the dry path.
	struct CabEntry
	{
		int row = -1;
		int KA = 0, KB = 0;           // taps of the IR the row has (fades to) / fades from; 0: dry
		const float* tapsA = nullptr; // device, padded with zeros to a multiple of four
		const float* tapsB = nullptr;
		int fading = 0;
		int N = 0, fk = 0;            // fade length, samples of it produced
		unsigned pos = 0;             // ring index the call's first sample goes to
		int hist = 0;                 // samples of the stream's history in front of it
	};

	class CabinetBook
	{
	public:
		// ---- set-up side ----
		static int RingFor(int taps)
		{
			int ring = 1;
			while (ring < taps - 1 + kCabPieceSamples) ring *= 2;
			return ring;
		}
		void Configure(int taps)
		{
			maxTaps = taps;
			ringSamples = RingFor(taps);
		}
		void Resize(int rowCount)
		{
			if (rowCount > (int)rows.size()) rows.resize((size_t)rowCount);
		}
		int Rows() const { return (int)rows.size(); }
		int MaxTaps() const { return maxTaps; }
		int RingSamples() const { return ringSamples; }
		int NumIRs() const { return numIRs; }
		// the lowest free id (ids of unloaded IRs are recycled)
		int AddIR(const float* deviceTaps, int K)
		{
			size_t id = 0;
			while (id < irs.size() && irs[id].K > 0) id++;
			if (id == irs.size()) irs.push_back(IR());
			irs[id].taps = deviceTaps;
			irs[id].K = K;
			irs[id].users = 0;
			numIRs++;
			return (int)id;
		}
		bool IsLoaded(int ir) const { return ir >= 0 && ir < (int)irs.size() && irs[(size_t)ir].K > 0; }
		int Users(int ir) const { return irs[(size_t)ir].users; }
		int Taps(int ir) const { return irs[(size_t)ir].K; }
		const float* RemoveIR(int ir)
		{
			const float* taps = irs[(size_t)ir].taps;
			irs[(size_t)ir] = IR();
			numIRs--;
			return taps;
		}
		int IRSlots() const { return (int)irs.size(); }
		const float* TapsOf(int ir) const { return irs[(size_t)ir].taps; }

		// ---- real-time side ----
		bool HasEntries() const { return numEntries > 0; }
		int NumEntries() const { return numEntries; }
		int Target(int s) const { return rows[(size_t)s].cur; }
		bool Fading(int s) const { return rows[(size_t)s].fading; }
		int FadeRemaining(int s) const { return rows[(size_t)s].fading ? rows[(size_t)s].N - rows[(size_t)s].k : 0; }

		// s: in no fade; ir: loaded or kCabDry; N >= 0
		void SetIR(int s, int ir, int N)
		{
			Row& r = rows[(size_t)s];
			if (r.cur == kCabDry)
			{
				if (ir == kCabDry) return;
				// T0: the history starts with the next sample
				r.pos = 0;
				r.hist = 0;
				numEntries++;
				Use(ir, +1);
				r.cur = ir;
				if (N > 0) BeginFade(r, kCabDry, N);
				return;
			}
			const int from = r.cur;
			r.cur = ir;
			Use(ir, +1);
			if (N > 0)
			{
				BeginFade(r, from, N); // (`from` keeps its user until the fade is over)
				return;
			}
			Use(from, -1);
			if (ir == kCabDry) Retire(r);
		}
		// park / removal: dry at once, the history is dropped
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (r.cur == kCabDry && !r.fading) return;
			Use(r.cur, -1);
			if (r.fading) Use(r.from, -1);
			r.cur = kCabDry;
			r.fading = false;
			Retire(r);
		}

		// the entries of the next call, into table[0 .. NumEntries()); returns how many
		int BuildTable(CabEntry* table) const
		{
			int count = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (r.cur == kCabDry && !r.fading) continue;
				CabEntry& e = table[count++];
				e.row = (int)s;
				e.KA = r.cur == kCabDry ? 0 : irs[(size_t)r.cur].K;
				e.tapsA = r.cur == kCabDry ? nullptr : irs[(size_t)r.cur].taps;
				e.fading = r.fading ? 1 : 0;
				e.KB = (!r.fading || r.from == kCabDry) ? 0 : irs[(size_t)r.from].K;
				e.tapsB = (!r.fading || r.from == kCabDry) ? nullptr : irs[(size_t)r.from].taps;
				e.N = r.N;
				e.fk = r.k;
				e.pos = r.pos;
				e.hist = r.hist;
			}
			return count;
		}

		// `n` samples were produced with the table BuildTable made: rings and fades move on, a fade that produced its last sample ends
		// (its `from` IR is free again), a stream that has faded to dry retires
		void Advance(size_t n)
		{
			if (numEntries == 0) return;
			for (Row& r : rows)
			{
				if (r.cur == kCabDry && !r.fading) continue;
				r.pos = (unsigned)(((unsigned long long)r.pos + n) & (unsigned long long)(ringSamples - 1));
				r.hist = (int)std::min<unsigned long long>((unsigned long long)(maxTaps - 1), (unsigned long long)r.hist + n);
				if (!r.fading) continue;
				r.k = (int)std::min<unsigned long long>((unsigned long long)r.N, (unsigned long long)r.k + n);
				if (r.k < r.N) continue;
				Use(r.from, -1);
				r.fading = false;
				if (r.cur == kCabDry) Retire(r);
			}
		}

	private:
		struct Row
		{
			int cur = kCabDry, from = kCabDry; // the IR the row has (fades to), the one it fades from
			bool fading = false;
			int N = 0, k = 0;
			unsigned pos = 0;
			int hist = 0;
		};
		struct IR
		{
			const float* taps = nullptr;
			int K = 0; // 0: a free id
			int users = 0;
		};
		void Use(int ir, int d)
		{
			if (ir != kCabDry) irs[(size_t)ir].users += d;
		}
		static void BeginFade(Row& r, int from, int N)
		{
			r.from = from;
			r.fading = true;
			r.N = N;
			r.k = 0;
		}
		void Retire(Row& r)
		{
			r = Row();
			numEntries--;
		}
		std::vector<Row> rows;
		std::vector<IR> irs;
		int maxTaps = 0, ringSamples = 0, numIRs = 0, numEntries = 0;
	};

	// (cabinet_stage_kernels.hip) the launches of one piece over `count` entries of the device table: `n` samples of every row from
	// sample `done` of the call on, rows `stride` floats apart, in place; rings `ringSamples` floats apart
	struct CabLaunch
	{
		const CabEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long done;
		int n;
		float* rings;
		int ringSamples;
	};

	unsigned long long CabinetStageLaunches(); // launches of the stage's kernels so far (NA_DebugCabinetLaunches)
}
