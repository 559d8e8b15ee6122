// room_stage.cpp -- the batch's side of the room stage (gpu_batch.h, room_stage.h): the rules of the calls, the lifetime
// of rings, setting blocks and tables, and the one upload + one launch a processing call with entries enqueues.  The arithmetic and
// the bookkeeping are in room_stage.h; the stage's place in the chain is GpuBatch::StageId (gpu_batch.h), what every stage shares is in
// gpu_batch_internal.h.
#include "gpu_batch_internal.h"

namespace na
{
	namespace
	{
		constexpr size_t kRoomSettingFloats = sizeof(RoomSetting) / sizeof(float);
	}

	GpuBatch::RoomStage::~RoomStage()
	{
		if (rings) (void)CountedHipFree(rings);
		if (settings) (void)CountedHipFree(settings);
	}

	void GpuBatch::EnableRoomStage(int maxLineSamples)
	{
		CheckUsable();
		if (maxLineSamples < kRoomMinMaxLine || maxLineSamples > kRoomMaxLineSamples || (maxLineSamples & (maxLineSamples - 1)) != 0)
			throw std::runtime_error("neuralaudio_amd: EnableRoomStage: maxLineSamples must be a power of two in [256, 16384]");
		CheckHip(hipSetDevice(device), "hipSetDevice");
		if (!stages[kRoomStage]) stages[kRoomStage].reset(new RoomStage());
		RoomStage& st = Require<RoomStage>("EnableRoomStage");
		if (maxLineSamples > st.book.MaxLine())
		{
			if (st.book.HasEntries()) throw std::runtime_error("neuralaudio_amd: EnableRoomStage: a larger maxLineSamples is refused while a stream has a room");
			if (st.rings)
			{
				// (no stream has a room: no history to carry over; the launches that read the old rings are over before they go)
				Quiesce();
				(void)CountedHipFree(st.rings);
				st.rings = nullptr;
				st.ringRows = 0;
			}
			st.book.Configure(maxLineSamples);
		}
		EnableStage<RoomStage>();
	}

	// set-up side (EnableRoomStage, CreateStreams): eight rings and a setting block per row, tables that hold what every row can put into
	// one call -- its entry and its setting
	void GpuBatch::RoomStage::EnsureRows(GpuBatch& batch, int rows)
	{
		book.Resize(rows);
		const int want = std::max(rows, 16);
		tables.Ensure(batch, want * kRoomRowUnits);
		if (want > ringRows)
		{
			// the rows that exist keep their histories: whatever reads or writes the old block is over before it is copied
			if (rings) batch.Quiesce();
			batch.GrowRowBlock(rings, (size_t)kRoomLines * (size_t)book.RingSamples(), ringRows, want, "hipMalloc (room rings)", "room rings");
			ringRows = want;
		}
		if (want > settingRows)
		{
			if (settings) batch.Quiesce();
			float* block = reinterpret_cast<float*>(settings);
			batch.GrowRowBlock(block, kRoomSettingFloats, settingRows, want, "hipMalloc (room settings)", "room settings");
			settings = reinterpret_cast<RoomSetting*>(block);
			settingRows = want;
		}
	}

	RoomStageInfo GpuBatch::GetRoomInfo() const
	{
		const RoomStage& st = Require<RoomStage>("GetRoomInfo");
		RoomStageInfo info;
		info.maxLineSamples = st.book.MaxLine();
		info.ringSamples = st.book.RingSamples();
		info.pieceSamples = kRoomPieceSamples;
		info.numRooms = st.book.NumEntries();
		info.deviceBytes = (long long)st.ringRows * kRoomLines * st.book.RingSamples() * (long long)sizeof(float) + (long long)st.settingRows * (long long)sizeof(RoomSetting)
			+ st.tables.Bytes();
		return info;
	}

	void GpuBatch::SetStreamRoom(int s, const RoomParams* params, int fadeSamples)
	{
		RoomBook& book = SettableStage<RoomStage>(s, "SetStreamRoom").book;
		if (params)
			if (const char* why = RoomParamsError(*params, book.MaxLine()))
				throw std::runtime_error(std::string("neuralaudio_amd: SetStreamRoom: ") + why + " (maxLineSamples = " + std::to_string(book.MaxLine()) + ")");
		RequireFadeRange(fadeSamples, "SetStreamRoom", "fadeSamples");
		if (book.Fading(s))
			throw std::runtime_error("neuralaudio_amd: SetStreamRoom: a room fade of " + StreamId(s) + " is running (" + std::to_string(book.FadeRemaining(s)) + " samples left)");
		book.Set(s, params, fadeSamples);
	}

	bool GpuBatch::GetStreamRoom(int s, RoomParams& out) const
	{
		const RoomStage& st = Require<RoomStage>("GetStreamRoom");
		RequireRow(s, "GetStreamRoom");
		if (!st.book.HasRoom(s)) return false;
		out = st.book.Target(s);
		return true;
	}

	int GpuBatch::StreamRoomFadeRemaining(int s) const
	{
		const RoomStage& st = Require<RoomStage>("StreamRoomFadeRemaining");
		RequireRow(s, "StreamRoomFadeRemaining");
		return st.book.FadeRemaining(s);
	}

	// Behind the delay stage and in front of the reverb stage, on the stream the models ran on: the table of this call's entries -- and
	// behind them the settings of the set calls since the last call: `units`, not `count`, go up -- from the next pinned table of the ring
	// (the wait for the launch that read it is bounded), ONE launch runs every entry's pieces, and the host mirror moves on by the n
	// samples the caller sees.
	void GpuBatch::RoomStage::Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride)
	{
		if (n == 0) return;
		tables.Require(book.Rows() <= ringRows && book.Rows() <= settingRows);
		const auto table = tables.Take(batch, book.NumEntries() * kRoomRowUnits);
		int units = 0;
		const int count = book.BuildTable(table.host, units);
		if (count > 0)
		{
			tables.Upload(table, units, launch);
			CheckHip(LaunchRoomStage(RoomLaunch{ table.dev, count, dOut, outStride, (unsigned long long)n, rings, book.RingSamples(), settings }, launch), "RoomStageKernel");
			tables.Commit(launch);
		}
		book.Advance(n);
	}

	void GpuBatch::DebugRunRoomStage(float* hostRows, long stride, size_t n)
	{
		CheckUsable();
		DebugRunStage(Require<RoomStage>("DebugRunRoomStage"), "DebugRunRoomStage", hostRows, stride, n);
	}
}
