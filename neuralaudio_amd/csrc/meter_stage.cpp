// meter_stage.cpp -- the batch's side of the meter stage (gpu_batch.h, meter_stage.h): the rules of the calls, the lifetime
// of the state block, the tables and the result blocks, the one upload + two launches + one result copy a processing call with entries
// enqueues, and the result path -- the only device -> host path of the stages: event queries and a fold into the book, never a wait.
// The arithmetic and the bookkeeping are in meter_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what
// every stage shares is in gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::MeterStage::~MeterStage()
	{
		if (state) (void)CountedHipFree(state);
	}

	void GpuBatch::EnableMeterStage() { EnableStage<MeterStage>(); }

	// set-up side (EnableMeterStage, CreateStreams): a state per row, tables that hold an entry per row and result blocks that hold a
	// record per entry
	void GpuBatch::MeterStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		results.Ensure(batch, want); // (the meters whose records are given up publish again with their next window)
		tables.Ensure(batch, want);
		if (want > rowCapacity)
		{
			// the rows that exist keep their states: whatever reads or writes the old block is over before it is copied
			if (state) batch.Quiesce();
			static_assert(sizeof(MeterState) == 44 * sizeof(float), "a state row is 44 words");
			static_assert(sizeof(MeterRecord) == 96 && sizeof(MeterEntry) == 32, "the records and entries the kernels read and write");
			batch.GrowRowBlock(state, sizeof(MeterState) / sizeof(float), rowCapacity, want, "hipMalloc (meter state)", "meter state");
			rowCapacity = want;
		}
	}

	MeterStageInfo GpuBatch::GetMeterInfo() const
	{
		const MeterStage& st = Require<MeterStage>("GetMeterInfo");
		MeterStageInfo info;
		info.numMeters = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * (long long)sizeof(MeterState) + st.tables.Bytes() + st.results.Bytes();
		return info;
	}

	void GpuBatch::SetStreamMeter(int s, const MeterParams* params)
	{
		MeterBook& book = SettableStage<MeterStage>(s, "SetStreamMeter").book;
		if (!params)
		{
			book.Remove(s);
			return;
		}
		if (const char* why = MeterParamsError(*params)) throw std::runtime_error(std::string("neuralaudio_amd: SetStreamMeter: ") + why);
		book.Set(s, *params);
	}

	bool GpuBatch::GetStreamMeter(int s, MeterParams& out) const
	{
		const MeterStage& st = Require<MeterStage>("GetStreamMeter");
		RequireRow(s, "GetStreamMeter");
		if (!st.book.HasMeter(s)) return false;
		out = st.book.Params(s);
		return true;
	}

	// real-time safe: event queries and host copies
	bool GpuBatch::ReadStreamMeter(int s, MeterReading& out)
	{
		CheckUsable();
		MeterStage& st = Require<MeterStage>("ReadStreamMeter");
		RequireRow(s, "ReadStreamMeter");
		st.Poll();
		if (!st.book.HasReading(s)) return false;
		out = st.book.Latest(s);
		return true;
	}

	// the pinned entry table of the same ring slot still says which row each record belongs to; a record of a meter that has been set
	// again or taken away since carries another generation and is dropped (MeterBook::Accept)
	void GpuBatch::MeterStage::Fold(int i, int records)
	{
		for (int k = 0; k < records; k++)
		{
			const MeterRecord& rec = results.host[i][k];
			if (rec.row == tables.host[i][k].row) (void)book.Accept(rec);
		}
	}

	// In front of the model launches, on the stream the call runs on: what has arrived is folded, the table of this call's entries goes up
	// from the next pinned table of the ring (the wait for the launch that read it is bounded; its records are folded before they are
	// overwritten) and the IN tap reads the input rows as the caller passed them -- they may be the output rows.  The gate stage is in
	// front of this one in StageId order: its table for the call is built, so which meter entries are gated in this call is known here.
	void GpuBatch::MeterStage::BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride)
	{
		count = 0;
		Poll();
		tables.Require(book.Rows() <= rowCapacity && book.NumEntries() <= results.capacity);
		const auto table = tables.Take(batch, book.NumEntries());
		slot = tables.next;
		results.FoldBlock(slot, [this](int i, int records) { Fold(i, records); });
		const int entries = book.BuildTable(table.host);
		if (entries == 0) return;
		const GateStage* gate = static_cast<const GateStage*>(batch.stages[kGateStage].get());
		anyGated = false;
		if (gate && gate->HasEntries())
			for (int k = 0; k < entries; k++)
			{
				table.host[k].gated = gate->book.IsEntry(table.host[k].row) ? 1 : 0;
				anyGated = anyGated || table.host[k].gated != 0;
			}
		tables.Upload(table, entries, launch);
		CheckHip(LaunchMeterIn(MeterLaunch{ table.dev, entries, dIn, inStride, (unsigned long long)n, nullptr, 0, reinterpret_cast<MeterState*>(state), nullptr }, launch),
			"MeterTapKernel (in)");
		count = entries;
		dev = table.dev;
	}

	// Behind the output stage: the OUT and GATE taps read the rows the caller receives and the gate's gain block of this call, the
	// records go to the pinned block of the table's ring slot, the table's event covers the copy, the ring moves on and the host mirror
	// by the n samples the caller sees.
	void GpuBatch::MeterStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		if (count == 0) return;
		const GateStage* gate = static_cast<const GateStage*>(batch.stages[kGateStage].get());
		// (the gate's own Run is over: its book may have retired an entry with this call, its gain block still holds the call's gains)
		const float* gains = (gate && anyGated) ? gate->gains : nullptr;
		const long gainSamples = (gate && anyGated) ? (long)gate->gainSamples : 0;
		CheckHip(LaunchMeterOut(MeterLaunch{ dev, count, dOut, outStride, (unsigned long long)n, gains, gainSamples, reinterpret_cast<MeterState*>(state), results.dev[slot] }, launch),
			"MeterTapKernel (out)");
		results.Download(slot, count, launch, "hipMemcpyAsync (meter results)");
		tables.Commit(launch);
		count = 0;
		book.Advance(n);
	}
}
