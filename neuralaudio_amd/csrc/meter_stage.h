// meter_stage.h -- the per-stream meter stage of a batch: level meters on the row a stream takes in (the IN tap) and on
// the row its caller receives (the OUT tap), and a gain-reduction meter on what the gate stage did to it (the GATE tap)
// (NA_BatchEnableMeterStage / NA_BatchSetStreamMeter / NA_BatchReadStreamMeter).  It never writes an audio row.  No reference
// counterpart: a host of the reference meters the buffers it holds; here the rows stay on the device.
//
// This header is the host bookkeeping, the table entry and the records the kernels read and write (meter_stage_kernels.hip) and the
// functions both sides run: MeterSample (one sample into a partial), MeterMerge (two partials) and MeterFold -- the ONE function that
// folds a run of samples into a tap's state and publishes on a window boundary.  It uses no HIP, so that it compiles and runs on its
// own.  All of it is index arithmetic on arrays sized on the set-up side (Resize): the real-time calls -- Set, Remove, Leave, BuildTable,
// Advance, Accept -- allocate nothing.
//
// Unlike the gate this stage is NOT a recurrence: every quantity is a max, a min or an integer sum, so the result does not depend on the
// order of evaluation, on how the signal is cut into calls, on alignment or on stride, and the kernels put lanes along the samples.
//
// Arithmetic (the contract of include/neuralaudio_amd.h).  Positions count the samples the caller sees since the meter was set,
// W = windowSamples, window k covers positions [kW, (k+1)W).  For each sample of a tap:
//   x' = (x is NaN) ? 0 : min(|x|, 1e18f)
//   q  = (unsigned) trunc(min(x', 8.0f) * 2^21)     (the product is exact; q <= 2^24)
//   peak   = max(peak, x')        over the window      (exact; subnormals kept)
//   energy = energy + q * q       over the window, unsigned 64-bit    (<= 2^63 for W <= 32768)
//   overs  = overs + (x' >= clipLevel ? 1 : 0)   over the window
//   peakHold   = max over every sample since the meter was set
//   oversTotal = overs summed over every sample since the meter was set (64-bit)
// For the GATE tap, g the gain the gate stage applied to the sample (1 where it applied none):
//   gateGainMin  = min(g) over the window
//   gateGainLast = g of the window's last sample
// A reading is published when a window completes; peakHold and oversTotal of a reading run through the end of its window.  x', the
// clip level and g are non-negative floats: their order is the order of their bit patterns as integers, and that is how max, min and
// >= are taken here -- no float instruction that could flush a subnormal sees them.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NA_METER_HD __host__ __device__ __forceinline__
#else
#define NA_METER_HD inline
#endif

namespace na
{
	constexpr int kMeterMinWindow = 32;
	constexpr int kMeterMaxWindow = 32768;
	constexpr uint32_t kMeterAbsLimitBits = 0x5D5E0B6Bu; // 1e18f
	constexpr uint32_t kMeterOneBits = 0x3F800000u;      // 1.0f: the g of a sample no gate touched
	constexpr uint32_t kMeterNoGainBits = 0xFFFFFFFFu;   // the identity of min over bit patterns
	enum : int { kMeterStartNone = 0, kMeterStartFresh = 1 };

	// the constants of a meter as the caller gives them (NA_MeterParams)
	struct MeterParams
	{
		int windowSamples = 1024;
		float clipLevelIn = 1.0f, clipLevelOut = 1.0f;
	};

	// nullptr: fine; else the text of the first rule the constants break (it names the field)
	inline const char* MeterParamsError(const MeterParams& p)
	{
		if (p.windowSamples < kMeterMinWindow || p.windowSamples > kMeterMaxWindow) return "windowSamples must lie in [32, 32768]";
		if (!std::isfinite(p.clipLevelIn) || !(p.clipLevelIn > 0.0f)) return "clipLevelIn must be finite and > 0";
		if (!std::isfinite(p.clipLevelOut) || !(p.clipLevelOut > 0.0f)) return "clipLevelOut must be finite and > 0";
		return nullptr;
	}

	NA_METER_HD uint32_t MeterBits(float f)
	{
		uint32_t b;
		__builtin_memcpy(&b, &f, 4);
		return b;
	}
	NA_METER_HD float MeterFloat(uint32_t b)
	{
		float f;
		__builtin_memcpy(&f, &b, 4);
		return f;
	}

	// One unit of work of the stage's launches: a row and its meter (32 bytes).  `start`: the state the call begins from is not the stored
	// one but that of a meter set since the last call (no memset travels with a set call).  `gen` is echoed in the record the call
	// produces, so that the host can tell a record of an earlier meter on the row from one of this meter.
	struct MeterEntry
	{
		int row = -1;
		int window = 0;
		uint32_t clipInBits = 0, clipOutBits = 0;
		int start = kMeterStartNone;
		uint32_t gen = 0;
		int gated = 0; // the row is an entry of the gate stage in this call: the GATE tap reads its gain row (else 1 for every sample)
		int reserved = 0;
	};

	// a tap's published window (NA_MeterTap, field for field)
	struct MeterTapReading
	{
		unsigned long long energy = 0, oversTotal = 0;
		float peak = 0.0f, peakHold = 0.0f;
		unsigned int overs = 0, reserved = 0;
	};
	// a meter's newest published window (NA_MeterReading, field for field)
	struct MeterReading
	{
		unsigned long long windows = 0;
		MeterTapReading in, out;
		float gateGainMin = 1.0f, gateGainLast = 1.0f;
		int windowSamples = 0, reserved = 0;
	};

	// what a run of samples comes to: the partial of a lane, of a wave, of a run
	struct MeterPartial
	{
		uint32_t peakBits = 0, overs = 0;
		uint32_t energyLo = 0, energyHi = 0; // the 64-bit sum as two words
	};

	// (lo, hi) += (addLo, addHi): the carry out of the low word goes into the high one
	NA_METER_HD void MeterAdd64(uint32_t& lo, uint32_t& hi, uint32_t addLo, uint32_t addHi)
	{
		const uint32_t sum = lo + addLo;
		const uint32_t carry = sum < addLo ? 1u : 0u;
		lo = sum;
		hi = hi + addHi + carry;
	}

	// one sample: the contract above, line by line
	NA_METER_HD void MeterSample(MeterPartial& p, float x, uint32_t clipBits)
	{
		uint32_t b = MeterBits(x) & 0x7FFFFFFFu;            // |x|
		if (b > 0x7F800000u) b = 0u;                        // NaN: 0
		if (b > kMeterAbsLimitBits) b = kMeterAbsLimitBits; // min(|x|, 1e18f), +inf included
		const float xa = MeterFloat(b);
		const float xs = xa < 8.0f ? xa : 8.0f;
		const uint32_t q = (uint32_t)(xs * 2097152.0f); // (a power of two: exact; a subnormal gives 0 flushed or not)
		const unsigned long long sq = (unsigned long long)q * (unsigned long long)q;
		if (b > p.peakBits) p.peakBits = b;
		MeterAdd64(p.energyLo, p.energyHi, (uint32_t)sq, (uint32_t)(sq >> 32));
		p.overs += b >= clipBits ? 1u : 0u;
	}

	NA_METER_HD void MeterMerge(MeterPartial& a, const MeterPartial& b)
	{
		if (b.peakBits > a.peakBits) a.peakBits = b.peakBits;
		a.overs += b.overs;
		MeterAdd64(a.energyLo, a.energyHi, b.energyLo, b.energyHi);
	}

	// a tap of a row, on the device (40 bytes): the window that is being filled, the holds and totals, the position
	struct MeterTapState
	{
		uint32_t energyLo = 0, energyHi = 0;
		unsigned long long oversTotal = 0;
		unsigned long long windows = 0;
		uint32_t peakBits = 0, holdBits = 0, overs = 0;
		uint32_t pos = 0; // samples of the window so far, < W
	};

	// per row, on the device (176 bytes).  The IN launch owns `in` and latest.in, the OUT launch everything else.
	struct MeterState
	{
		MeterTapState in, out;
		uint32_t gateMinBits = kMeterNoGainBits; // of the window that is being filled
		uint32_t gen = 0;
		MeterReading latest; // the newest published window (windows == 0: none yet)
	};

	// what a call's OUT launch leaves per entry, and the result copy brings to the host (96 bytes)
	struct MeterRecord
	{
		int row = -1;
		uint32_t gen = 0;
		MeterReading reading;
	};

	// the samples of the next run of a tap at position `pos` of its window: to the window's end or the call's
	NA_METER_HD uint32_t MeterRunLength(uint32_t pos, uint32_t W, unsigned long long left)
	{
		const uint32_t room = W - pos;
		return left < (unsigned long long)room ? (uint32_t)left : room;
	}

	// the state a call starts from: a start code replaces the stored state
	NA_METER_HD MeterTapState MeterBegin(const MeterEntry& e, const MeterTapState& s) { return e.start == kMeterStartFresh ? MeterTapState() : s; }

	// THE function of the stage: a run of `len` samples that ends at or before its window's end, summed up in `run`, joins the tap's
	// state; true: the window is complete -- `pub` holds its reading, the holds and totals have taken it in, a new window begins
	NA_METER_HD bool MeterFold(MeterTapState& s, const MeterPartial& run, uint32_t len, uint32_t W, MeterTapReading& pub)
	{
		if (run.peakBits > s.peakBits) s.peakBits = run.peakBits;
		s.overs += run.overs;
		MeterAdd64(s.energyLo, s.energyHi, run.energyLo, run.energyHi);
		s.pos += len;
		if (s.pos < W) return false;
		if (s.peakBits > s.holdBits) s.holdBits = s.peakBits;
		s.oversTotal += s.overs;
		s.windows += 1;
		pub.energy = ((unsigned long long)s.energyHi << 32) | (unsigned long long)s.energyLo;
		pub.oversTotal = s.oversTotal;
		pub.peak = MeterFloat(s.peakBits);
		pub.peakHold = MeterFloat(s.holdBits);
		pub.overs = s.overs;
		pub.reserved = 0;
		s.energyLo = s.energyHi = 0;
		s.peakBits = 0;
		s.overs = 0;
		s.pos = 0;
		return true;
	}

	class MeterBook
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
		bool HasMeter(int s) const { return rows[(size_t)s].has; }
		const MeterParams& Params(int s) const { return rows[(size_t)s].params; }
		uint32_t Gen(int s) const { return rows[(size_t)s].gen; }
		bool HasReading(int s) const { return rows[(size_t)s].has && rows[(size_t)s].arrived; }
		const MeterReading& Latest(int s) const { return rows[(size_t)s].latest; }

		// p: valid (MeterParamsError).  The meter starts -- or starts again -- at the next sample, at position 0, under a new generation:
		// nothing an earlier meter of the row produced is read from here on
		void Set(int s, const MeterParams& p)
		{
			Row& r = rows[(size_t)s];
			if (!r.has)
			{
				r.has = true;
				numEntries++;
			}
			r.start = kMeterStartFresh;
			r.gen = ++lastGen;
			r.arrived = false;
			r.params = p;
		}
		// the meter goes at once: it touches no audio, so there is no tail
		void Remove(int s)
		{
			Row& r = rows[(size_t)s];
			if (!r.has) return;
			r = Row();
			r.gen = ++lastGen;
			numEntries--;
		}
		// park / removal of the stream: the same
		void Leave(int s) { Remove(s); }

		// the entries of the next call, into table[0 .. NumEntries()); returns how many (`gated` is the stage's to fill in)
		int BuildTable(MeterEntry* table) const
		{
			int count = 0;
			if (numEntries == 0) return 0;
			for (size_t s = 0; s < rows.size(); s++)
			{
				const Row& r = rows[s];
				if (!r.has) continue;
				MeterEntry& e = table[count++];
				e.row = (int)s;
				e.window = r.params.windowSamples;
				e.clipInBits = MeterBits(r.params.clipLevelIn);
				e.clipOutBits = MeterBits(r.params.clipLevelOut);
				e.start = r.start;
				e.gen = r.gen;
				e.gated = 0;
				e.reserved = 0;
			}
			return count;
		}

		// `n` samples were produced with the table BuildTable made: the start codes are spent
		void Advance(size_t n)
		{
			if (numEntries == 0 || n == 0) return;
			for (Row& r : rows)
				if (r.has) r.start = kMeterStartNone;
		}

		// a record has arrived on the host: it becomes the row's newest reading if it is this meter's (the generations agree) and holds a
		// completed window; true: taken
		bool Accept(const MeterRecord& rec)
		{
			if (rec.row < 0 || rec.row >= (int)rows.size()) return false;
			Row& r = rows[(size_t)rec.row];
			if (!r.has || r.gen != rec.gen || rec.reading.windows == 0) return false;
			r.latest = rec.reading;
			r.arrived = true;
			return true;
		}

	private:
		struct Row
		{
			bool has = false, arrived = false;
			int start = kMeterStartNone;
			uint32_t gen = 0;
			MeterParams params;
			MeterReading latest;
		};
		std::vector<Row> rows;
		int numEntries = 0;
		uint32_t lastGen = 0; // of the batch: a generation is never used twice (2^32 set calls apart)
	};

	// (meter_stage_kernels.hip) a tap launch over `count` entries of the device table: `n` samples of every entry's row, rows `stride`
	// floats apart.  The IN launch: the rows are the input rows; gains and results unused.  The OUT launch: the rows the caller receives,
	// the gate stage's gain block of this call (rows `gainSamples` floats apart; nullptr: no entry is gated), and results[0 .. count)
	struct MeterLaunch
	{
		const MeterEntry* table;
		int count;
		const float* rows;
		long stride;
		unsigned long long n;
		const float* gains;
		long gainSamples;
		MeterState* state;
		MeterRecord* results;
	};

	unsigned long long MeterStageLaunches(); // launches of the stage's two kernels so far (NA_DebugMeterLaunches)
}
