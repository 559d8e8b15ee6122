// drive_stage.cpp -- the batch's side of the drive stage (gpu_batch.h, drive_stage.h): the rules of the calls, the
// lifetime of the history blocks, the coefficient block, the model-input block and the tables, and the one upload + one launch a
// processing call with entries enqueues in front of its model launches.  The arithmetic and the bookkeeping are in drive_stage.h; the
// stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what every stage shares is in gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	GpuBatch::DriveStage::~DriveStage()
	{
		if (history) (void)CountedHipFree(history);
		if (block) (void)CountedHipFree(block);
		if (coefs) (void)CountedHipFree(coefs);
	}

	void GpuBatch::EnableDriveStage()
	{
		CheckUsable();
		if (Resamples()) throw std::runtime_error("neuralaudio_amd: EnableDriveStage: the drive stage is refused on a resampling batch");
		EnableStage<DriveStage>();
	}

	// set-up side (EnableDriveStage, CreateStreams): the coefficients of the three factors, two history blocks and a row of the
	// model-input block per row, tables that hold an entry per row
	void GpuBatch::DriveStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want);
		if (!coefs)
		{
			std::vector<float> host((size_t)3 * kDriveCoefFloats);
			for (int L : { 2, 4, 8 }) DriveCoefBlock(L, host.data() + (size_t)DriveCoefSlot(L) * kDriveCoefFloats);
			CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&coefs), host.size() * sizeof(float)), "hipMalloc (drive coefficients)");
			CheckHip(hipMemcpy(coefs, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy (drive coefficients)");
		}
		if (want > rowCapacity)
		{
			// the rows that exist keep their histories: whatever reads or writes the old blocks is over before they are copied
			if (history) batch.Quiesce();
			batch.GrowRowBlock(history, (size_t)2 * kDriveHistory, rowCapacity, want, "hipMalloc (drive history)", "drive history");
			batch.GrowRowBlock(block, (size_t)blockSamples, 0, want, "hipMalloc (drive block)", "drive block"); // (nothing of the block outlives its call)
			rowCapacity = want;
		}
	}

	// a call longer than the block's rows: they grow (not real-time safe, like any first use of a longer buffer)
	void GpuBatch::DriveStage::EnsureSamples(GpuBatch& batch, size_t n)
	{
		if (n <= (size_t)blockSamples) return;
		if (n > (size_t)1 << 30) throw std::runtime_error("neuralaudio_amd: drive stage: the call is too long for the model-input block");
		int samples = blockSamples;
		while ((size_t)samples < n) samples *= 2;
		batch.Quiesce(); // (the model launches of an earlier call may still read the old block)
		batch.GrowRowBlock(block, (size_t)samples, 0, rowCapacity, "hipMalloc (drive block)", "drive block");
		blockSamples = samples;
	}

	DriveStageInfo GpuBatch::GetDriveInfo() const
	{
		const DriveStage& st = Require<DriveStage>("GetDriveInfo");
		DriveStageInfo info;
		info.numDrives = st.book.NumEntries();
		info.deviceBytes = (long long)st.rowCapacity * ((long long)st.blockSamples + 2 * kDriveHistory) * (long long)sizeof(float) + 3ll * kDriveCoefFloats * (long long)sizeof(float) + st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamDrive(int s, const DriveParams* params, int rampSamples)
	{
		DriveBook& book = SettableStage<DriveStage>(s, "SetStreamDrive").book;
		if (!params)
		{
			book.Remove(s);
			return;
		}
		if (const char* why = DriveParamsError(*params)) throw std::runtime_error(std::string("neuralaudio_amd: SetStreamDrive: ") + why);
		RequireFadeRange(rampSamples, "SetStreamDrive", "rampSamples");
		if (book.RampRemaining(s) > 0)
			throw std::runtime_error("neuralaudio_amd: SetStreamDrive: " + StreamId(s) + ": ramp running (" + std::to_string(book.RampRemaining(s)) + " samples left)");
		if (book.HasDrive(s) && book.Target(s).shape != params->shape)
			throw std::runtime_error("neuralaudio_amd: SetStreamDrive: shape belongs to the drive for its life (" + StreamId(s) + " has one: take it away first)");
		if (book.HasDrive(s) && book.Target(s).oversample != params->oversample)
			throw std::runtime_error("neuralaudio_amd: SetStreamDrive: oversample belongs to the drive for its life (" + StreamId(s) + " has one: take it away first)");
		book.Set(s, *params, rampSamples);
	}

	bool GpuBatch::GetStreamDrive(int s, DriveParams& out) const
	{
		const DriveStage& st = Require<DriveStage>("GetStreamDrive");
		RequireRow(s, "GetStreamDrive");
		if (!st.book.HasDrive(s)) return false;
		out = st.book.Target(s);
		return true;
	}

	int GpuBatch::StreamDriveRampRemaining(int s) const
	{
		const DriveStage& st = Require<DriveStage>("StreamDriveRampRemaining");
		RequireRow(s, "StreamDriveRampRemaining");
		return st.book.RampRemaining(s);
	}

	// In front of the model launches, on the stream the call runs on: the table of this call's rows goes up from the next pinned table of
	// the ring (the wait for the launch that read it is bounded), one launch reads the input rows as the caller passed them -- they may
	// be the output rows, and they are never written -- into the model-input block, and the host mirror moves on by the n samples the
	// caller sees.  ProcessDeviceOn hands the block to the model launches in place of the caller's rows (`filled`).
	void GpuBatch::DriveStage::BeforeModels(GpuBatch& batch, hipStream_t launch, const float* dIn, size_t n, long inStride)
	{
		filled = false;
		if (n == 0) return;
		const int rows = batch.NumStreams();
		tables.Require(rows <= rowCapacity && rows <= book.Rows());
		EnsureSamples(batch, n);
		const auto table = tables.Take(batch, rows);
		book.BuildTable(table.host, rows);
		tables.Upload(table, rows, launch);
		CheckHip(LaunchDriveStage(DriveLaunch{ table.dev, rows, dIn, inStride, block, (long)blockSamples, (unsigned long long)n, history, coefs }, launch), "DriveStageKernel");
		tables.Commit(launch);
		book.Advance(n);
		filled = true;
	}

	void GpuBatch::DriveStage::Run(GpuBatch&, hipStream_t, float*, size_t, long) {}
}
