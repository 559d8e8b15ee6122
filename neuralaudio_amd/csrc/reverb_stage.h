// reverb_stage.h -- the per-stream reverb stage of a batch: every stream that has a long impulse response (IR) gets its
// row replaced by dry * row + wet * (row convolved with the IR), behind the cabinet stage and in front of the output stage
// (NA_BatchEnableReverbStage / NA_BatchLoadReverbIR / NA_BatchSetStreamReverb).  The cabinet stage is direct form and ends at 8192 taps;
// this one is uniformly partitioned FFT convolution (overlap-save, partitions of P = 128 samples, 256-point transforms) and ends at
// 131072 taps.  No reference counterpart: a host of the reference convolves on the CPU.
//
// This header is the host bookkeeping, the table entry the kernels read (reverb_stage_kernels.hip) and the step functions of the
// arithmetic.  It uses no HIP, so that it compiles and runs on its own.  All of it is index arithmetic on arrays sized on the set-up side
// (Configure, Resize, AddIR): the real-time calls -- Set, BuildTable, Advance, Leave -- allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h).  Every operation below is ONE f32 operation, rounded to nearest even, never
// contracted into an FMA; f32 subnormals are kept (operands and results).  Positions t count from T0, the first sample after the set call
// that took the stream from dry; x[t] is the row's sample, x[t] = 0 for t < 0; block m is the samples [128 m, 128 m + 128).
//   twiddles    W[q] = (fl(cos(2 pi q / 256)), fl(-sin(2 pi q / 256))), q in [0, 128): computed in double, rounded once (ReverbTwiddles)
//   product     (a + bi)(c + di) = (fl(fl(a c) - fl(b d)), fl(fl(a d) + fl(b c)))                                        (RevMul)
//   transform   F(v), v of 256 complex values: the radix-2 decimation-in-time transform.  u[i] = v[bit-reversal of i in 8 bits]; then
//               for s = 1 .. 8, half = 2^(s-1), for every i in [0, 128): j = i mod half, top = 2 (i - j) + j, bot = top + half,
//               p = RevMul(W[j * 128 / half], u[bot]), u[bot] = u[top] - p, u[top] = u[top] + p (componentwise; ALL 256 complex bins
//               are carried, also where the input is real; the product is taken also where W = (1, 0)).  The inverse F' is the same with
//               the twiddles' imaginary parts negated (exact), without the scale.
//   head        head[t] = sum over k in [0, min(K, 128)) with k <= t, in rising k from +0, of h[k] * x[t - k]: acc = fl(acc + fl(h[k] x[t-k]))
//   spectra     X_m = F([x block m-1, x block m]) (imaginary parts +0);  H_j = F([h[128 j .. 128 j + 128), 128 zeros]), j = 1 .. J - 1,
//               J = ceil(K / 128), taps past K are +0
//   tail        A_b = sum over j in [1, min(J - 1, b)], in rising j from (+0, +0), of RevMul(H_j, X_{b-j}), componentwise acc = fl(acc + p);
//               tail[128 b + i] = fl(Re(F'(A_b))[128 + i] * 2^-8)   (exact scale)
//   output      c = fl(head + tail);  y = fl(fl(dry x) + fl(wet c))                                                       (RevMix)
//   fade        the k-th sample after a set call of length N from setting A to setting B: w = OutStageWeightAt(N, k); y_B itself where
//               w = 1, else fl(fl(fl(1 - w) y_A) + fl(w y_B)); the output of the dry setting (no reverb) is x itself        (RevBlend)
// Nothing of the call, the row, the launch, the other entries or maxTaps enters a sample's value.
//
// Device state per row: a ring of raw samples (kRevRingSamples: a piece and the 2 P samples in front of it), a ring of `slots` input
// spectra (the frequency-domain delay line; slot m mod slots holds X_m; slots = partitions of maxTaps - 1 + the blocks a piece can
// touch), and for each of the two settings of a fade the tails of the blocks a piece can touch.  What lies before T0 reads as zero by
// index, so nothing is cleared when a history is dropped.  The spectra do not depend on the IR: a switch of IR continues on the history
// the old one saw.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "output_stage.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_REV_HD __host__ __device__ __forceinline__
#else
#define NA_REV_HD inline
#endif

namespace na
{
	constexpr int kRevMaxTaps = 131072;
	constexpr int kRevPartition = 128;                 // P: samples of a partition, taps of the head
	constexpr int kRevPoints = 2 * kRevPartition;      // points of the transform
	constexpr int kRevSpectrumFloats = 2 * kRevPoints; // (re, im) of every bin
	constexpr int kRevPieceSamples = 1024;             // the longest run the stage processes at once
	constexpr int kRevPieceBlocks = kRevPieceSamples / kRevPartition + 1; // blocks a piece can touch
	constexpr int kRevRingSamples = 2048;              // raw samples per row: a power of two >= kRevPieceSamples + 2 P
	constexpr int kRevTailBlocks = 16;                 // tails kept per row and setting: a power of two >= kRevPieceBlocks
	constexpr int kRevTailFloats = 2 * kRevTailBlocks * kRevPartition; // per row
	constexpr int kRevDry = -1;                        // the IR id of "no reverb"
	static_assert(kRevRingSamples >= kRevPieceSamples + 2 * kRevPartition && (kRevRingSamples & (kRevRingSamples - 1)) == 0, "ring");
	static_assert(kRevTailBlocks >= kRevPieceBlocks && (kRevTailBlocks & (kRevTailBlocks - 1)) == 0, "tails");

	inline int RevPartitions(int K) { return (K + kRevPartition - 1) / kRevPartition; } // J, the head included
	// floats of an IR on the device: the head's 128 taps, then H_1 .. H_{J-1}
	inline size_t RevIRFloats(int K) { return (size_t)kRevPartition + (size_t)(RevPartitions(K) - 1) * kRevSpectrumFloats; }

	// the twiddle table, W[q] at [2q], [2q + 1]: computed once, in double, rounded to f32
	inline const float* ReverbTwiddles()
	{
		static const std::vector<float> table = [] {
			std::vector<float> w((size_t)kRevPoints);
			for (int q = 0; q < kRevPartition; q++)
			{
				const double a = 2.0 * 3.14159265358979323846 * (double)q / (double)kRevPoints;
				w[(size_t)(2 * q)] = (float)std::cos(a);
				w[(size_t)(2 * q + 1)] = (float)-std::sin(a);
			}
			return w;
		}();
		return table.data();
	}

	struct RevComplex
	{
		float re, im;
	};

	NA_REV_HD RevComplex RevMul(RevComplex a, RevComplex b)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float ac = a.re * b.re;
		const float bd = a.im * b.im;
		const float ad = a.re * b.im;
		const float bc = a.im * b.re;
		RevComplex p;
		p.re = ac - bd;
		p.im = ad + bc;
		return p;
	}

	NA_REV_HD RevComplex RevAdd(RevComplex a, RevComplex b)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		RevComplex s;
		s.re = a.re + b.re;
		s.im = a.im + b.im;
		return s;
	}

	NA_REV_HD RevComplex RevSub(RevComplex a, RevComplex b)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		RevComplex s;
		s.re = a.re - b.re;
		s.im = a.im - b.im;
		return s;
	}

	// one term of the head's sum
	NA_REV_HD float RevHeadStep(float acc, float h, float x)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float p = h * x;
		return acc + p;
	}

	NA_REV_HD float RevMix(float dry, float wet, float x, float head, float tail)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float c = head + tail;
		const float d = dry * x;
		const float v = wet * c;
		return d + v;
	}

	NA_REV_HD float RevBlend(float w, float from, float to)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (w == 1.0f) return to;
		const float u = 1.0f - w;
		const float a = u * from;
		const float b = w * to;
		return a + b;
	}

	// one setting of a row as the kernels see it
	struct RevSide
	{
		const float* ir = nullptr; // device: RevIRFloats(K) floats; nullptr: no reverb, the output is the row itself
		int K = 0;
		float wet = 0.0f, dry = 1.0f;
		int tails = 0;             // which of the row's two tail blocks this setting has
		int have = 0;              // the tail of the block that holds the call's first sample exists (it was computed by an earlier call)
	};

	// One unit of work of the stage's launches: a row, its setting and -- during a fade -- the setting it fades from
	struct RevEntry
	{
		int row = -1;
		int fading = 0;
		int N = 0, fk = 0;   // fade length, samples of it produced
		long long t = 0;     // position of the call's first sample, counted from T0
		RevSide to, from;
	};

	class ReverbBook
	{
	public:
		// ---- set-up side ----
		static int SlotsFor(int taps) { return RevPartitions(taps) - 1 + kRevPieceBlocks; }
		void Configure(int taps)
		{
			maxTaps = taps;
			slots = SlotsFor(taps);
		}
		void Resize(int rowCount)
		{
			if (rowCount > (int)rows.size()) rows.resize((size_t)rowCount);
		}
		int Rows() const { return (int)rows.size(); }
		int MaxTaps() const { return maxTaps; }
		int Slots() const { return slots; }
		int NumIRs() const { return numIRs; }
		// the lowest free id (ids of unloaded IRs are recycled)
		int AddIR(const float* deviceIR, int K)
		{
			size_t id = 0;
			while (id < irs.size() && irs[id].K > 0) id++;
			if (id == irs.size()) irs.push_back(IR());
			irs[id].data = deviceIR;
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
			const float* data = irs[(size_t)ir].data;
			irs[(size_t)ir] = IR();
			numIRs--;
			return data;
		}
		int IRSlots() const { return (int)irs.size(); }
		const float* DataOf(int ir) const { return irs[(size_t)ir].data; }

		// ---- real-time side ----
		bool HasEntries() const { return numEntries > 0; }
		int NumEntries() const { return numEntries; }
		int Target(int s) const { return rows[(size_t)s].cur.ir; }
		float TargetWet(int s) const { return rows[(size_t)s].cur.wet; }
		float TargetDry(int s) const { return rows[(size_t)s].cur.dry; }
		bool Fading(int s) const { return rows[(size_t)s].fading; }
		int FadeRemaining(int s) const { return rows[(size_t)s].fading ? rows[(size_t)s].N - rows[(size_t)s].k : 0; }

		// s: in no fade; ir: loaded or kRevDry; N >= 0
		void Set(int s, int ir, float wet, float dry, int N)
		{
			Row& r = rows[(size_t)s];
			Setting next;
			next.ir = ir;
			if (ir != kRevDry)
			{
				next.wet = wet;
				next.dry = dry;
			}
			if (r.cur.ir == kRevDry)
			{
				if (ir == kRevDry) return;
				// T0: the history starts with the next sample
				r.t = 0;
				numEntries++;
				Use(ir, +1);
				r.from = Setting();
				r.from.tails = 1;
				r.cur = next;
				if (N > 0) BeginFade(r, N);
				return;
			}
			Use(ir, +1);
			if (N > 0)
			{
				// (`from` keeps its user, its tails and what it has of them until the fade is over)
				next.tails = 1 - r.cur.tails;
				r.from = r.cur;
				r.cur = next;
				BeginFade(r, N);
				return;
			}
			Use(r.cur.ir, -1);
			next.tails = r.cur.tails;
			r.cur = next; // (the tail of the running block is the old IR's: the next call computes the new one's)
			if (ir == kRevDry) Retire(r);
		}
		// park / removal: no reverb at once, the history is dropped
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (r.cur.ir == kRevDry && !r.fading) return;
			Use(r.cur.ir, -1);
			if (r.fading) Use(r.from.ir, -1);
			r.fading = false;
			Retire(r);
		}

		// the entries of the next call, into table[0 .. NumEntries()); returns how many
		int BuildTable(RevEntry* table) const
		{
			int count = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (r.cur.ir == kRevDry && !r.fading) continue;
				RevEntry& e = table[count++];
				e.row = (int)s;
				e.fading = r.fading ? 1 : 0;
				e.N = r.N;
				e.fk = r.k;
				e.t = (long long)r.t;
				e.to = SideOf(r.cur);
				e.from = r.fading ? SideOf(r.from) : RevSide();
			}
			return count;
		}

		// what the launches of a piece of n samples at `done` samples into the call have to cover: the most blocks any entry completes
		// (spectrum launch) and the most blocks any entry needs a new tail for (tail launch)
		struct PieceNeeds
		{
			int spectra = 0, tails = 0;
		};
		PieceNeeds NeedsOf(size_t done, int n) const
		{
			PieceNeeds needs;
			for (const Row& r : rows)
			{
				if (r.cur.ir == kRevDry && !r.fading) continue;
				const unsigned long long t = r.t + done;
				const int o = (int)(t % (unsigned long long)kRevPartition);
				needs.spectra = std::max(needs.spectra, (o + n) / kRevPartition);
				const int touched = (o + n - 1) / kRevPartition + 1;
				// (the tail of a block that began before the piece exists, unless a set call since then brought a setting that lacks it)
				const bool firstExists = o != 0 && AllSidesHave(r, done);
				needs.tails = std::max(needs.tails, touched - (firstExists ? 1 : 0));
			}
			return needs;
		}

		// `n` samples were produced with the table BuildTable made: positions and fades move on, a fade that produced its last sample
		// ends (its `from` IR is free again), a stream that has faded to dry retires
		void Advance(size_t n)
		{
			if (numEntries == 0) return;
			for (Row& r : rows)
			{
				if (r.cur.ir == kRevDry && !r.fading) continue;
				r.t += n;
				r.cur.have = true;
				r.from.have = true;
				if (!r.fading) continue;
				r.k = (int)std::min<unsigned long long>((unsigned long long)r.N, (unsigned long long)r.k + n);
				if (r.k < r.N) continue;
				Use(r.from.ir, -1);
				r.fading = false;
				if (r.cur.ir == kRevDry) Retire(r);
			}
		}

	private:
		struct Setting
		{
			int ir = kRevDry;
			float wet = 0.0f, dry = 1.0f;
			int tails = 0;
			bool have = false;
		};
		struct Row
		{
			Setting cur, from; // the setting the row has (fades to), the one it fades from
			bool fading = false;
			int N = 0, k = 0;
			unsigned long long t = 0;
		};
		struct IR
		{
			const float* data = nullptr;
			int K = 0; // 0: a free id
			int users = 0;
		};
		static bool AllSidesHave(const Row& r, size_t done)
		{
			if (done > 0) return true;
			if (r.cur.ir != kRevDry && !r.cur.have) return false;
			if (r.fading && r.from.ir != kRevDry && !r.from.have) return false;
			return true;
		}
		RevSide SideOf(const Setting& g) const
		{
			RevSide side;
			if (g.ir == kRevDry) return side;
			side.ir = irs[(size_t)g.ir].data;
			side.K = irs[(size_t)g.ir].K;
			side.wet = g.wet;
			side.dry = g.dry;
			side.tails = g.tails;
			side.have = g.have ? 1 : 0;
			return side;
		}
		void Use(int ir, int d)
		{
			if (ir != kRevDry) irs[(size_t)ir].users += d;
		}
		static void BeginFade(Row& r, int N)
		{
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
		int maxTaps = 0, slots = 0, numIRs = 0, numEntries = 0;
	};

	// (reverb_stage_kernels.hip) the launches of one piece over `count` entries of the device table: `n` samples of every row from
	// sample `done` of the call on, rows `stride` floats apart, in place
	struct RevLaunch
	{
		const RevEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long done;
		int n;
		const float* twiddles; // device: kRevPoints floats
		float* rings;          // [row][kRevRingSamples]
		float* spectra;        // [row][slots][kRevSpectrumFloats]
		float* tails;          // [row][2][kRevTailBlocks][kRevPartition]
		int slots;
		int spectrumBlocks, tailBlocks; // ReverbBook::NeedsOf: 0: no such launch
	};

	// (reverb_stage_kernels.hip) load side: H_1 .. H_{J-1} of the `taps` on the device (J * 128 floats, zeros behind the IR's last tap) into `ir`
	struct RevIRLaunch
	{
		const float* taps;
		float* ir;
		int partitions; // J
		const float* twiddles;
	};

	unsigned long long ReverbStageLaunches(); // launches of the stage's kernels on the processing side so far (NA_DebugReverbLaunches)
}
