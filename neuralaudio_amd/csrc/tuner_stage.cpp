// tuner_stage.cpp -- the batch's side of the tuner stage (gpu_batch.h, tuner_stage.h): the rules of the calls, the
// lifetime of the state block, the rings, the tables and the result blocks, what a processing call with entries enqueues -- one upload,
// one append launch per piece and, in a call that holds an evaluation end, one evaluate launch and one result copy -- and the result
// path, which is the meter stage's (meter_stage.cpp): event queries and a fold into the book, never a wait.  The arithmetic and the
// bookkeeping are in tuner_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h).
#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::TunerStage::~TunerStage()
	{
		if (state) (void)CountedHipFree(state);
		if (rings) (void)CountedHipFree(rings);
	}

	void GpuBatch::EnableTunerStage() { EnableStage<TunerStage>(); }

	// set-up side (EnableTunerStage, CreateStreams): a state and a ring per row, tables that hold an entry per row and result blocks that
	// hold a record per entry
	void GpuBatch::TunerStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		results.Ensure(batch, want); // (the tuners whose records are given up evaluate again a hop later)
		tables.Ensure(batch, want);
		if (want > rowCapacity)
		{
			// the rows that exist keep their states and rings: whatever reads or writes the old blocks is over before they are copied
			if (state) batch.Quiesce();
			static_assert(sizeof(TunerState) == 2 * sizeof(float) && sizeof(int) == sizeof(float), "a state row is 2 words, a ring value one");
			static_assert(sizeof(TunerRecord) == 88 && sizeof(TunerEntry) == 72 && sizeof(TunerReading) == 80, "the records and entries the kernels read and write");
			batch.GrowRowBlock(state, sizeof(TunerState) / sizeof(float), rowCapacity, want, "hipMalloc (tuner state)", "tuner state");
			batch.GrowRowBlock(rings, (size_t)kTunerRingSamples, rowCapacity, want, "hipMalloc (tuner rings)", "tuner rings");
			rowCapacity = want;
		}
	}

	TunerStageInfo GpuBatch::GetTunerInfo() const
	{
		const TunerStage& st = Require<TunerStage>("GetTunerInfo");
		TunerStageInfo info;
		info.numTuners = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * ((long long)sizeof(TunerState) + (long long)kTunerRingSamples * (long long)sizeof(int)) + st.tables.Bytes() + st.results.Bytes();
		return info;
	}

	void GpuBatch::SetStreamTuner(int s, const TunerParams* params)
	{
		TunerBook& book = SettableStage<TunerStage>(s, "SetStreamTuner").book;
		if (!params)
		{
			book.Remove(s);
			return;
		}
		if (const char* why = TunerParamsError(*params)) throw std::runtime_error(std::string("neuralaudio_amd: SetStreamTuner: ") + why);
		book.Set(s, *params);
	}

	bool GpuBatch::GetStreamTuner(int s, TunerParams& out) const
	{
		const TunerStage& st = Require<TunerStage>("GetStreamTuner");
		RequireRow(s, "GetStreamTuner");
		if (!st.book.HasTuner(s)) return false;
		out = st.book.Params(s);
		return true;
	}

	// real-time safe: event queries and host copies
	bool GpuBatch::ReadStreamTuner(int s, TunerReading& out)
	{
		CheckUsable();
		TunerStage& st = Require<TunerStage>("ReadStreamTuner");
		RequireRow(s, "ReadStreamTuner");
		st.Poll();
		if (!st.book.HasReading(s)) return false;
		out = st.book.Latest(s);
		return true;
	}

	// the pinned entry table of the same ring slot still says which entry -- and so which row -- each record belongs to; a record of a
	// tuner that has been set again or taken away since carries another generation and is dropped (TunerBook::Accept)
	void GpuBatch::TunerStage::Fold(int i, int records)
	{
		const TunerEntry* table = tables.host[i];
		for (int k = 0; k < records; k++)
		{
			const TunerRecord& rec = results.host[i][k];
			const int entry = table[k].evalEntry;
			if (entry >= 0 && entry < tables.capacity && rec.row == table[entry].row) (void)book.Accept(rec);
		}
	}

	// In front of the model launches, on the stream the call runs on, behind the meter's IN tap (StageId order): what has arrived is
	// folded, the table of this call's entries goes up from the next pinned table of the ring (the wait for the launch that read it is
	// bounded; its records are folded before they are overwritten), every piece of the call is appended to the rings and -- where the
	// last evaluation end of an entry lies in the piece -- evaluated; the records go to the pinned block of the table's ring slot, the
	// table's event covers the copy, the ring moves on and the host mirror by the n samples the caller sees.  The rows are read as the
	// caller passed them -- they may be the output rows -- so all of it is here and nothing is left for Run.
	void GpuBatch::TunerStage::BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride)
	{
		Poll();
		if (n == 0) return;
		tables.Require(book.Rows() <= rowCapacity && book.NumEntries() <= results.capacity);
		const auto table = tables.Take(batch, book.NumEntries());
		const int slot = tables.next;
		results.FoldBlock(slot, [this](int i, int records) { Fold(i, records); });
		int evaluating = 0;
		const int entries = book.BuildTable(table.host, (unsigned long long)n, &evaluating);
		if (entries == 0) return;
		tables.Upload(table, entries, launch);
		TunerLaunch L{ table.dev, entries, evaluating, dIn, inStride, 0ull, 0ull, reinterpret_cast<TunerState*>(state), reinterpret_cast<int*>(rings), results.dev[slot] };
		for (size_t done = 0; done < n; done += (size_t)kTunerPieceSamples)
		{
			L.offset = (unsigned long long)done;
			L.n = (unsigned long long)std::min<size_t>((size_t)kTunerPieceSamples, n - done);
			CheckHip(LaunchTunerAppend(L, launch), "TunerAppendKernel");
			// (a call of one piece -- every call a real-time host makes -- asks nothing: all its evaluation ends lie in it)
			bool here = evaluating > 0 && n <= (size_t)kTunerPieceSamples;
			for (int k = 0; k < evaluating && !here; k++)
			{
				const TunerEntry& e = table.host[table.host[k].evalEntry];
				const unsigned long long last = (unsigned long long)(e.evalM + 1) * (unsigned long long)e.decimation - 1ull - e.pos; // in the call
				here = last >= L.offset && last < L.offset + L.n;
			}
			if (here) CheckHip(LaunchTunerEvaluate(L, launch), "TunerEvaluateKernel");
		}
		if (evaluating > 0) results.Download(slot, evaluating, launch, "hipMemcpyAsync (tuner results)");
		tables.Commit(launch);
		book.Advance(n);
	}

	void GpuBatch::TunerStage::Run(GpuBatch&, hipStream_t, float*, size_t, long) {}
}
