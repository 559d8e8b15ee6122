// drive_stage.h -- the per-stream drive stage of a batch: a boost or overdrive IN FRONT of the model -- a static
// nonlinearity between an L-fold oversampling FIR pair -- the one stage that changes what a model reads (NA_BatchEnableDriveStage /
// NA_BatchSetStreamDrive).  No reference counterpart: a host of the reference runs its pedals on the buffers it holds; here the rows
// stay on the device.
//
// This header is the host bookkeeping, the table entry the kernel reads (drive_stage_kernels.hip), the prototype filter and the ramp
// both sides evaluate.  It uses no HIP, so that it compiles and runs on its own.  All of it is index arithmetic on arrays sized on the
// set-up side (Resize): the real-time calls -- Set, Remove, Leave, BuildTable, Advance -- allocate nothing.
//
// Arithmetic (the contract of include/neuralaudio_amd.h).  L = oversample, T = 32, N = L T.  The prototype h[0 .. N] is computed in
// double -- h[j] ~ sinc((j - N/2) / L) I0(9 sqrt(1 - (2 (j - N/2) / N)^2)) / I0(9), normalised to sum 1 -- and rounded to f32.  Positions
// n = 0, 1, ... count the samples of the stream's input row since the set call that created the entry; x[n] = 0 for n < 0; a NaN reads as 0.
//   u[L n + p] = sum over t >= 0, p + L t <= N, ascending t, of (L h[p + L t]) x[n - t]          (p = 0 .. L-1; acc = fmaf(c, x, acc))
//   s[m]       = shape(g u[m] + b) - shape(b)                    (product, add, subtraction each rounded; g, b those of sample m / L)
//   w[n]       = sum over j = 0 .. N, ascending j, of h[j] s[L n - j]                                       (acc = fmaf(h, s, acc))
//   out[n]     = level * (mix * w[n] + (1 - mix) * x[n - T])                                       (every operation rounded by itself)
// Each sum is ONE f32 accumulator that starts at 0, every step of it one fused multiply-add; nothing else is fused.
// Ramp: k counts the samples since the LAST set call (negative behind it).  A value is `from` for k < 0, `to` for k >= R - 1 and
// from + (to - from) * ((float)(k + 1) / (float)R) between; the outputs between two set calls are those of the earlier one's ramp,
// which reaches back over the 2 T samples it still reads with its from-values.  k is advanced by whole calls and never accumulated.
// The kernel recomputes the s it reads from the 2 T input samples behind the call (kept per row), so a sample's bits do not depend on
// how the signal is cut into calls, on the stride or on the other streams.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace na
{
	constexpr int kDriveTaps = 32;                // T: taps per phase, and the stage's latency in samples at every L
	constexpr int kDriveHistory = 2 * kDriveTaps; // the input samples behind a call the stage keeps per row (two blocks of them: one read, one written)
	constexpr int kDriveMaxOversample = 8;
	constexpr int kDriveMaxRamp = 1 << 20;
	constexpr int kDriveMinBlockSamples = 1024;   // the model-input block's rows, a power of two, grown by a longer call
	enum : int { kDriveShapeTanh = 0, kDriveShapeCubic = 1, kDriveShapeHard = 2, kDriveCopy = -1 };
	// the coefficient block of one L on the device: h[0 .. N] ascending, then the up filter phase-major: up[p][t] = L h[p + L t]
	constexpr int kDriveDownFloats = kDriveMaxOversample * kDriveTaps + 8;
	constexpr int kDriveUpStride = kDriveTaps + 4;
	constexpr int kDriveCoefFloats = kDriveDownFloats + kDriveMaxOversample * kDriveUpStride;
	constexpr int DriveCoefSlot(int L) { return L == 2 ? 0 : (L == 4 ? 1 : 2); }

	// the constants of a drive as the caller gives them (NA_DriveParams, field for field)
	struct DriveParams
	{
		int shape = kDriveShapeTanh, oversample = 4;
		float drive = 1.0f, bias = 0.0f, mix = 1.0f, level = 1.0f;
		int reserved[2] = { 0, 0 };
	};

	// nullptr: fine; else the text of the first rule the constants break (it names the field)
	inline const char* DriveParamsError(const DriveParams& p)
	{
		if (p.shape < 0 || p.shape > 2) return "shape must lie in [0, 2]";
		if (p.oversample != 2 && p.oversample != 4 && p.oversample != 8) return "oversample must be 2, 4 or 8";
		if (!std::isfinite(p.drive) || p.drive < 0.0f || p.drive > 1000.0f) return "drive must be finite and lie in [0, 1000]";
		if (!std::isfinite(p.bias) || p.bias < -4.0f || p.bias > 4.0f) return "bias must be finite and lie in [-4, 4]";
		if (!(p.mix >= 0.0f && p.mix <= 1.0f)) return "mix must lie in [0, 1]";
		if (!std::isfinite(p.level) || p.level < 0.0f || p.level > 16.0f) return "level must be finite and lie in [0, 16]";
		return nullptr;
	}

	// the prototype of oversampling factor L in double, h[0 .. L T], normalised to sum 1
	inline std::vector<double> DrivePrototype(int L)
	{
		const auto I0 = [](double v) {
			double sum = 1.0, term = 1.0;
			for (int k = 1; k < 64; k++)
			{
				term *= (v / (2.0 * k)) * (v / (2.0 * k));
				sum += term;
			}
			return sum;
		};
		const int N = L * kDriveTaps;
		const double pi = 3.14159265358979323846;
		std::vector<double> h((size_t)N + 1);
		double sum = 0.0;
		for (int j = 0; j <= N; j++)
		{
			const double c = (double)(j - N / 2), a = pi * c / (double)L, r = 2.0 * c / (double)N;
			h[(size_t)j] = (c == 0.0 ? 1.0 : std::sin(a) / a) * I0(9.0 * std::sqrt(std::max(0.0, 1.0 - r * r))) / I0(9.0);
			sum += h[(size_t)j];
		}
		for (double& v : h) v /= sum;
		return h;
	}

	// the device block of factor L (kDriveCoefFloats floats; what the sums never read is 0)
	inline void DriveCoefBlock(int L, float* out)
	{
		const std::vector<double> h = DrivePrototype(L);
		const int N = L * kDriveTaps;
		for (int i = 0; i < kDriveCoefFloats; i++) out[i] = 0.0f;
		for (int j = 0; j <= N; j++)
		{
			const float f = (float)h[(size_t)j];
			out[j] = f;
			out[kDriveDownFloats + (j % L) * kDriveUpStride + j / L] = (float)L * f; // (a power of two: exact)
		}
	}

	// a ramped value at sample k of its ramp (k < 0: behind the set call)
#if defined(__HIPCC__) || defined(__CUDACC__)
	__host__ __device__ __forceinline__
#else
	inline
#endif
	float DriveRampAt(float from, float to, int R, long long k)
	{
		if (k < 0) return from;
		if (k >= (long long)R - 1) return to;
		const float w = (float)(k + 1) / (float)R; // (both exact in f32: the quotient is the double quotient rounded once)
		const float d = to - from, m = d * w;
		return from + m;
	}

	// One row of the stage's launch (64 bytes); the table holds one per row of the batch.  shape == kDriveCopy: the row has no drive and
	// is copied.  `fresh`: the call's first sample is position 0 of the entry -- the row's history block is not this entry's and reads
	// as zeros (no memset travels with a set call).  `parity`: which of the row's two history blocks the call reads; it writes the other.
	// `done`: samples since the last set call, at the call's first sample.  from / to: drive, bias, mix, level.
	struct DriveEntry
	{
		int shape = kDriveCopy, oversample = 0, fresh = 0, parity = 0, R = 0, reserved = 0;
		long long done = 0;
		float from[4] = { 0, 0, 0, 0 }, to[4] = { 0, 0, 0, 0 };
	};
	static_assert(sizeof(DriveEntry) == 64, "the entry the kernel reads");

	class DriveBook
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
		bool HasDrive(int s) const { return rows[(size_t)s].has; }
		const DriveParams& Target(int s) const { return rows[(size_t)s].params; }
		int RampRemaining(int s) const
		{
			const Row& r = rows[(size_t)s];
			return r.has && r.done < (long long)r.R ? (int)((long long)r.R - r.done) : 0;
		}

		// p: valid (DriveParamsError), no ramp running, shape and oversample those of the entry if there is one.  A new entry starts at
		// the next sample, at position 0, from drive and bias of p, mix 0 and level 1: the delayed dry row
		void Set(int s, const DriveParams& p, int rampSamples)
		{
			Row& r = rows[(size_t)s];
			const float to[4] = { p.drive, p.bias, p.mix, p.level };
			if (!r.has)
			{
				const bool parity = r.parity;
				r = Row();
				r.parity = parity;
				r.has = true;
				numEntries++;
				const float from[4] = { p.drive, p.bias, 0.0f, 1.0f };
				for (int i = 0; i < 4; i++) r.from[i] = rampSamples > 0 ? from[i] : to[i];
			}
			else
				for (int i = 0; i < 4; i++) r.from[i] = r.to[i]; // (no ramp is running: the values in effect are the last targets)
			for (int i = 0; i < 4; i++) r.to[i] = to[i];
			r.R = rampSamples;
			r.done = 0;
			r.params = p;
			r.params.reserved[0] = r.params.reserved[1] = 0;
		}
		// the drive goes at once, with its history: the model reads the row undelayed from the next call on
		void Remove(int s)
		{
			Row& r = rows[(size_t)s];
			if (!r.has) return;
			const bool parity = r.parity;
			r = Row();
			r.parity = parity;
			numEntries--;
		}
		// park / removal of the stream: the same
		void Leave(int s) { Remove(s); }

		// the rows of the next call, into table[0 .. rowCount): one entry per row of the batch
		void BuildTable(DriveEntry* table, int rowCount) const
		{
			for (int s = 0; s < rowCount; s++)
			{
				DriveEntry e;
				const Row& r = rows[(size_t)s];
				if (r.has)
				{
					e.shape = r.params.shape;
					e.oversample = r.params.oversample;
					e.fresh = r.pos == 0 ? 1 : 0;
					e.parity = r.parity ? 1 : 0;
					e.R = r.R;
					e.done = r.done;
					for (int i = 0; i < 4; i++)
					{
						e.from[i] = r.from[i];
						e.to[i] = r.to[i];
					}
				}
				table[s] = e;
			}
		}

		// `n` samples were taken with the table BuildTable made
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				r.pos += n;
				r.done += (long long)n;
				r.parity = !r.parity;
			}
		}

	private:
		struct Row
		{
			bool has = false, parity = false;
			int R = 0;
			long long done = 0;         // samples since the last set call
			unsigned long long pos = 0; // samples the entry has taken
			float from[4] = { 0, 0, 0, 0 }, to[4] = { 0, 0, 0, 0 };
			DriveParams params;
		};
		std::vector<Row> rows;
		int numEntries = 0;
	};

	// (drive_stage_kernels.hip) the launch of one call: samples [0, n) of all `rows` rows of the batch (`in` points at the call's first
	// sample; rows `inStride` floats apart) into the model-input block `out` (rows `outStride` floats apart): a driven row processed, the
	// others copied.  history: [rows][2][kDriveHistory]; coefs: [3][kDriveCoefFloats] (DriveCoefSlot)
	struct DriveLaunch
	{
		const DriveEntry* table;
		int rows;
		const float* in;
		long inStride;
		float* out;
		long outStride;
		unsigned long long n;
		float* history;
		const float* coefs;
	};

	unsigned long long DriveStageLaunches(); // launches of the stage's kernel so far (NA_DebugDriveLaunches)
}
