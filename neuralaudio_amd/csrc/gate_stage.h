// gate_stage.h -- the per-stream gate stage of a batch: a noise gate that listens to a stream's dry input row and scales
// the row the models produced for it, in front of the cabinet and output stages (NA_BatchEnableGateStage / NA_BatchSetStreamGate).  No
// reference counterpart: a host of the reference gates its sessions itself, because it holds both buffers; here the rows stay on the
// device.
//
// This header is the host bookkeeping, the table entry the kernels read (gate_stage_kernels.hip) and the ONE step function both sides
// run.  It uses no HIP, so that it compiles and runs on its own.  All of it is index arithmetic on arrays sized on the set-up side
// (Resize): the real-time calls -- Set, Remove, Leave, BuildTable, Advance -- allocate nothing.
//
// Unlike the other two stages this one is a recurrence: a level follower, a hysteresis state machine with hold, and a slewed gain.  Its
// state (GateState) lives on the device and is carried from call to call; the host mirror keeps the constants and counts samples.
//
// Arithmetic (the contract of include/neuralaudio_amd.h): separately rounded f32 operations in this order, no FMA contraction
// (GateStep below, compiled with contraction off).  Constants of an entry: a detector coefficient, Po >= Pc open / close thresholds as
// power, H hold, A / R attack / release lengths in samples, floor the gain of the closed gate; span = fl(1 - floor), U = 2^30,
// stepUp = ceil(U / A), stepDown = ceil(U / R).  State: f32 p, integer hold, bit open, unsigned u in [0, U].  Per sample, x the input
// sample, y the row's sample after the models:
//   x' = (x is NaN) ? 0 : min(|x|, 1e18f)
//   s = fl(x' * x');  d = fl(s - p);  p = fl(p + fl(a * d))
//   if      p >= Po:  open = 1, hold = H
//   else if p <  Pc:  if hold > 0: hold -= 1  else: open = 0
//   u = open ? min(U, u + stepUp) : (u > stepDown ? u - stepDown : 0)
//   g = (u == U) ? 1.0f : fl(floor + fl(span * fl((float)u * 2^-30)))
//   y = fl(y * g)
// A gate that is being taken away (forceOpen) runs the same step with `open` forced to 1 in front of the line that moves u -- the
// follower and the hold counter go on as they would, so that a set call during the tail finds the state it would have had.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_GATE_HD __host__ __device__ __forceinline__
#else
#define NA_GATE_HD inline
#endif

namespace na
{
	constexpr unsigned kGateUnit = 1u << 30;       // U: the gain position of the open gate
	constexpr int kGateMaxSlew = 1 << 20;          // attackSamples, releaseSamples
	constexpr int kGateMaxHold = 1 << 24;          // holdSamples
	constexpr int kGateMinGainSamples = 2048;      // the gain block's first row length (a power of two; a longer call grows it)
	enum : int { kGateStartNone = 0, kGateStartOpen = 1, kGateStartClosed = 2 };

	// the constants of a gate as the caller gives them (NA_GateParams)
	struct GateParams
	{
		float openPower = 0.0f, closePower = 0.0f, floorGain = 0.0f, detectorCoeff = 1.0f;
		int attackSamples = 1, holdSamples = 0, releaseSamples = 1;
	};

	// nullptr: fine; else the text of the first rule the constants break (it names the field)
	inline const char* GateParamsError(const GateParams& p)
	{
		if (!std::isfinite(p.openPower)) return "openPower must be finite";
		if (!std::isfinite(p.closePower)) return "closePower must be finite";
		if (!std::isfinite(p.floorGain)) return "floorGain must be finite";
		if (!std::isfinite(p.detectorCoeff)) return "detectorCoeff must be finite";
		if (p.closePower < 0.0f) return "closePower must be >= 0";
		if (p.openPower < p.closePower) return "openPower must be >= closePower";
		if (p.floorGain < 0.0f || p.floorGain > 1.0f) return "floorGain must lie in [0, 1]";
		if (!(p.detectorCoeff > 0.0f) || p.detectorCoeff > 1.0f) return "detectorCoeff must lie in (0, 1]";
		if (p.attackSamples < 1 || p.attackSamples > kGateMaxSlew) return "attackSamples must lie in [1, 1 << 20]";
		if (p.holdSamples < 0 || p.holdSamples > kGateMaxHold) return "holdSamples must lie in [0, 1 << 24]";
		if (p.releaseSamples < 1 || p.releaseSamples > kGateMaxSlew) return "releaseSamples must lie in [1, 1 << 20]";
		return nullptr;
	}

	// NA_GateParamsFromDb: thresholds are dBFS of a sine's peak (power = 10^(dB/10) / 2), the floor is 10^(dB/20) (-inf: 0), the detector
	// coefficient 1 - exp(-1 / (ms * rate / 1000)) in double, rounded once; sample counts max(1, round(ms * rate / 1000)), hold may be 0.
	// nullptr: fine; else what is wrong.
	inline const char* GateParamsFromDb(int sampleRate, float openDb, float closeDb, float floorDb, float detectorMs, float attackMs, float holdMs, float releaseMs,
		GateParams& out)
	{
		if (sampleRate < 1) return "sampleRate must be >= 1";
		if (!std::isfinite(openDb)) return "openPower must be finite";
		if (!std::isfinite(closeDb)) return "closePower must be finite";
		if (std::isnan(floorDb) || floorDb == INFINITY) return "floorGain must be finite";
		if (!std::isfinite(detectorMs) || !(detectorMs > 0.0f)) return "detectorCoeff must lie in (0, 1]";
		if (!std::isfinite(attackMs) || !std::isfinite(releaseMs) || !std::isfinite(holdMs))
			return !std::isfinite(attackMs) ? "attackSamples must lie in [1, 1 << 20]" : (!std::isfinite(holdMs) ? "holdSamples must lie in [0, 1 << 24]" : "releaseSamples must lie in [1, 1 << 20]");
		const double rate = (double)sampleRate;
		const auto count = [&](float ms, double least) {
			const double c = std::max(least, std::floor((double)ms * rate / 1000.0 + 0.5));
			return (int)std::min(c, 2147483647.0);
		};
		GateParams p;
		p.openPower = (float)(std::pow(10.0, (double)openDb / 10.0) / 2.0);
		p.closePower = (float)(std::pow(10.0, (double)closeDb / 10.0) / 2.0);
		p.floorGain = floorDb == -INFINITY ? 0.0f : (float)std::pow(10.0, (double)floorDb / 20.0);
		p.detectorCoeff = (float)(1.0 - std::exp(-1.0 / ((double)detectorMs * rate / 1000.0)));
		p.attackSamples = count(attackMs, 1.0);
		p.holdSamples = count(holdMs, 0.0);
		p.releaseSamples = count(releaseMs, 1.0);
		if (const char* why = GateParamsError(p)) return why;
		out = p;
		return nullptr;
	}

	// the constants the step reads
	struct GateConsts
	{
		float a = 1.0f, Po = 0.0f, Pc = 0.0f, floor = 0.0f, span = 1.0f;
		int H = 0;
		unsigned stepUp = kGateUnit, stepDown = kGateUnit;
	};
	inline GateConsts GateConstsOf(const GateParams& p)
	{
		GateConsts c;
		c.a = p.detectorCoeff;
		c.Po = p.openPower;
		c.Pc = p.closePower;
		c.floor = p.floorGain;
		c.span = 1.0f - p.floorGain;
		c.H = p.holdSamples;
		c.stepUp = (kGateUnit + (unsigned)p.attackSamples - 1u) / (unsigned)p.attackSamples;
		c.stepDown = (kGateUnit + (unsigned)p.releaseSamples - 1u) / (unsigned)p.releaseSamples;
		return c;
	}

	// One unit of work of the stage's launches: a row and its gate.  `start`: the state the call begins from is not the stored one but
	// the open / closed start of a gate set since the last call (no memset travels with a set call).
	struct GateEntry
	{
		int row = -1;
		GateConsts c;
		int start = kGateStartNone;
		int forceOpen = 0; // the gate is being taken away: `open` is forced to 1
	};

	// per row, on the device (16 bytes)
	struct GateState
	{
		float p = 0.0f;
		int hold = 0;
		int open = 0;
		unsigned u = 0;
	};

	// the state a call starts from: a start code replaces the stored state; new constants keep it, with hold = min(hold, H)
	NA_GATE_HD GateState GateBegin(const GateEntry& e, GateState s)
	{
		if (e.start == kGateStartOpen)
		{
			s.p = 0.0f;
			s.hold = e.c.H;
			s.open = 1;
			s.u = kGateUnit;
		}
		else if (e.start == kGateStartClosed)
		{
			s.p = 0.0f;
			s.hold = 0;
			s.open = 0;
			s.u = 0u;
		}
		if (s.hold > e.c.H) s.hold = e.c.H;
		return s;
	}

	NA_GATE_HD float GateGainOf(const GateConsts& c, unsigned u)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		if (u == kGateUnit) return 1.0f;
		const float pos = (float)u * 9.31322574615478515625e-10f; // 2^-30: exact scaling of the rounded u
		const float part = c.span * pos;
		return c.floor + part;
	}

	// one sample: the contract above, line by line; returns g
	NA_GATE_HD float GateStep(const GateConsts& c, int forceOpen, GateState& s, float x)
	{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
		const float xa = (x != x) ? 0.0f : fminf(fabsf(x), 1e18f);
		const float sq = xa * xa;
		const float d = sq - s.p;
		const float ad = c.a * d;
		s.p = s.p + ad;
		if (s.p >= c.Po)
		{
			s.open = 1;
			s.hold = c.H;
		}
		else if (s.p < c.Pc)
		{
			if (s.hold > 0) s.hold -= 1;
			else s.open = 0;
		}
		const bool open = s.open != 0 || forceOpen != 0;
		if (forceOpen) s.open = 1;
		if (open) s.u = (s.u + c.stepUp > kGateUnit) ? kGateUnit : s.u + c.stepUp; // (u + stepUp <= 2^31: no wrap)
		else s.u = s.u > c.stepDown ? s.u - c.stepDown : 0u;
		return GateGainOf(c, s.u);
	}

	class GateBook
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
		// a gate that is not being taken away
		bool HasGate(int s) const { return rows[(size_t)s].has && !rows[(size_t)s].removing; }
		bool IsEntry(int s) const { return rows[(size_t)s].has; }
		const GateParams& Params(int s) const { return rows[(size_t)s].params; }
		int Start(int s) const { return rows[(size_t)s].start; }
		int RemovalRemaining(int s) const { return rows[(size_t)s].removing ? rows[(size_t)s].left : 0; }

		// p: valid (GateParamsError).  No gate: it starts at the next sample, open or closed.  A gate (also one being taken away): the
		// new constants from the next sample on the kept state; startOpen is ignored.
		void Set(int s, const GateParams& p, bool startOpen)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				r.has = true;
				r.start = startOpen ? kGateStartOpen : kGateStartClosed;
				numEntries++;
			}
			r.removing = false;
			r.left = 0;
			r.params = p;
		}
		// click-free: the entry stays, forced open, for attackSamples samples -- u == U by then, by construction (stepUp * A >= U)
		void Remove(int s)
		{
			Row& r = rows[(size_t)s];
			if (!r.has || r.removing) return;
			r.removing = true;
			r.left = r.params.attackSamples;
		}
		// park / removal of the stream: the gate goes at once
		void Leave(int s)
		{
			Row& r = rows[(size_t)s];
			if (!r.has) return;
			r = Row();
			numEntries--;
		}

		// the entries of the next call, into table[0 .. NumEntries()); returns how many
		int BuildTable(GateEntry* table) const
		{
			int count = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				GateEntry& e = table[count++];
				e.row = (int)s;
				e.c = GateConstsOf(r.params);
				e.start = r.start;
				e.forceOpen = r.removing ? 1 : 0;
			}
			return count;
		}

		// `n` samples were produced with the table BuildTable made: the start codes are spent, removals that have produced their
		// attackSamples samples retire
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
			{
				if (!r.has) continue;
				r.start = kGateStartNone;
				if (!r.removing) continue;
				r.left -= (int)std::min<unsigned long long>((unsigned long long)r.left, (unsigned long long)n);
				if (r.left > 0) continue;
				r = Row();
				numEntries--;
			}
		}

	private:
		struct Row
		{
			bool has = false, removing = false;
			int start = kGateStartNone;
			int left = 0; // samples the removal still has to produce
			GateParams params;
		};
		std::vector<Row> rows;
		int numEntries = 0;
	};

	// (gate_stage_kernels.hip) the detector launch over `count` entries of the device table: `n` input samples of every entry's row, rows
	// `inStride` floats apart; the gains go to gains[row][0 .. n), rows `gainSamples` floats apart; the state of every entry moves on
	struct GateDetectLaunch
	{
		const GateEntry* table;
		int count;
		const float* in;
		long inStride;
		unsigned long long n;
		float* gains;
		long gainSamples;
		GateState* state;
	};
	// ... and the apply launch: rows[row][i] *= gains[row][i], in place
	struct GateApplyLaunch
	{
		const GateEntry* table;
		int count;
		float* rows;
		long stride;
		unsigned long long n;
		const float* gains;
		long gainSamples;
	};

	unsigned long long GateStageLaunches(); // launches of the stage's two kernels so far (NA_DebugGateLaunches)
}
