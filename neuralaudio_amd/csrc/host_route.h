// host_route.h -- how a buffer gets onto the device: which route each of the four processing entry points of GpuBatch takes
// (ProcessHost, ProcessHostToDevice, Submit, ProcessDevice), given plain facts about the batch and the call (DESIGN.md 2.4 "Routes").
// Host data only: no HIP header, no environment, no device, so that the rule compiles and is tested on its own
// (tests/test_host_route_cpu.py).  An entry point gathers its facts, asks, and switches on the answer; a stage never touches this rule --
// "any stage has entries" is one of its facts.
#pragma once

namespace na
{
	// every route of the four entry points; the values are what NA_DebugLastHostRoute reports
	enum class HostRoute
	{
		// ProcessHost (blocking)
		RegisteredInPlace, // blocks the caller registered: the kernels run on them as they are, on the batch stream
		StagedHalves,      // through the pinned staging block, each chain's rows staged, launched and copied out by themselves
		StagedInPlace,     // through the pinned staging block, which the kernels read and write themselves
		StagedCopies,      // through the pinned staging block and its device twin: upload, kernels, download on the batch stream
		// Submit
		SubmitHalves,      // the slot's pinned blocks in place, on the free-running chains
		SubmitInPlace,     // the slot's pinned blocks in place, on the batch stream
		SubmitOwnStream,   // upload, kernel and download on the slot's own stream
		SubmitCopyStreams, // upload on the copy-in stream, kernels on the batch stream, download on the copy-out stream
		// ProcessDevice
		DeviceResident,    // a command to the resident launch
		DeviceHalves,      // the free-running chains
		DeviceOrdered,     // on the batch stream, behind everything launched so far
		// ProcessHostToDevice
		ToDeviceInPlace,   // the kernels read the pinned staging block themselves
		ToDeviceCopies,    // the staging block is uploaded in front of them
		kCount
	};

	// "Direct": the kernels read and write a pinned host block themselves instead of the copy engines.  Not while a stage has entries:
	// the stages work in place on device memory, not as a read-modify-write over the bus.
	inline bool DirectRows(bool hostDirect, bool stageEntries) { return hostDirect && !stageEntries; }

	// ---- ProcessHost ----
	struct BlockingFacts
	{
		bool hostDirect;        // the host-direct knob is on (Tuning::hostDirect)
		bool stageEntries;      // any stage has entries
		bool bothRegistered;    // `in` and `out` both lie inside blocks the caller registered
		bool pinnedAddressable; // the device can address the pinned staging block (asked only of a call that stages, and is direct)
		bool rowRangesOnly;     // the half lists just prepared are contiguous row ranges: the host can stage a half by itself
	};
	// the call needs no staging block
	inline bool BlockingRunsOnCallersBlocks(const BlockingFacts& f) { return DirectRows(f.hostDirect, f.stageEntries) && f.bothRegistered; }
	inline bool BlockingStagedDirect(const BlockingFacts& f) { return DirectRows(f.hostDirect, f.stageEntries) && f.pinnedAddressable; }
	// the call runs PrepareHalves
	inline bool BlockingTriesHalves(const BlockingFacts& f) { return !BlockingRunsOnCallersBlocks(f) && BlockingStagedDirect(f); }
	inline HostRoute BlockingRouteFor(const BlockingFacts& f, bool halvesPrepared)
	{
		if (BlockingRunsOnCallersBlocks(f)) return HostRoute::RegisteredInPlace;
		if (BlockingTriesHalves(f) && halvesPrepared && f.rowRangesOnly) return HostRoute::StagedHalves;
		return BlockingStagedDirect(f) ? HostRoute::StagedInPlace : HostRoute::StagedCopies;
	}

	// ---- ProcessHostToDevice: it alone does not look at the stages (its output rows are device memory, only the input crosses the bus) ----
	struct ToDeviceFacts
	{
		bool hostDirect;
		bool pinnedAddressable; // the staging block (asked only with the knob on)
	};
	inline HostRoute ToDeviceRouteFor(const ToDeviceFacts& f) { return f.hostDirect && f.pinnedAddressable ? HostRoute::ToDeviceInPlace : HostRoute::ToDeviceCopies; }

	// ---- Submit ----
	struct SubmitFacts
	{
		bool hostDirect;
		bool stageEntries;
		bool resamples;           // the batch resamples: three ordered launches per buffer
		bool pinnedAddressable;   // the device can address both pinned blocks of the slot (asked only of a direct call)
		bool callerPassedIn;      // `in` != nullptr: the library copies the caller's rows (nullptr: NextInput was filled in place)
		bool otherTicketInFlight; // another slot is busy
		bool chainsInUse;         // the chain streams may hold work of this batch
		int launchUnits;          // launch units of a buffer (launch_plan.h)
	};
	inline bool SubmitDirect(const SubmitFacts& f) { return DirectRows(f.hostDirect, f.stageEntries) && f.pinnedAddressable; }
	// the call runs PrepareHalves.  A lone buffer gains nothing from being split, so only with another ticket in flight (or the chains
	// already running); nor does a submission whose rows the library copies: the host thread is the bottleneck there.
	inline bool SubmitTriesHalves(const SubmitFacts& f) { return SubmitDirect(f) && !f.callerPassedIn && (f.otherTicketInFlight || f.chainsInUse); }
	inline HostRoute SubmitRouteFor(const SubmitFacts& f, bool halvesPrepared)
	{
		if (SubmitTriesHalves(f) && halvesPrepared) return HostRoute::SubmitHalves;
		if (SubmitDirect(f)) return HostRoute::SubmitInPlace;
		// one launch per buffer rides on the slot's own stream; several units (a fork / join or a captured graph) and the three launches
		// of a resampling batch run on the batch stream
		return f.launchUnits <= 1 && !f.resamples ? HostRoute::SubmitOwnStream : HostRoute::SubmitCopyStreams;
	}

	// ---- ProcessDevice ----
	struct DeviceFacts
	{
		bool ownsStream;     // the batch created its stream ...
		bool streamObserved; // ... and has handed it out (or it is the caller's): the order of work on it can be seen from outside
		bool resamples;
		bool stageEntries;
	};
	// the call runs TryResident and, if that declines, PrepareHalves: nobody can observe the order of work on streams they never saw.
	// Not a call that runs ordered on ONE stream: a resampling batch, a batch whose stages have entries.
	inline bool DeviceTriesFreeRunning(const DeviceFacts& f) { return f.ownsStream && !f.streamObserved && !(f.resamples || f.stageEntries); }
	inline HostRoute DeviceRouteFor(const DeviceFacts& f, bool residentTook, bool halvesPrepared)
	{
		if (DeviceTriesFreeRunning(f) && residentTook) return HostRoute::DeviceResident;
		if (DeviceTriesFreeRunning(f) && halvesPrepared) return HostRoute::DeviceHalves;
		return HostRoute::DeviceOrdered;
	}

	// what Collect waits for: written by Submit's arm
	enum class SlotWait
	{
		ChainEvents,     // SubmitHalves: the slot's halfDone events
		OwnStream,       // SubmitOwnStream: the download is the stream's last operation
		DownloadedEvent, // SubmitInPlace, SubmitCopyStreams: the slot's `downloaded` event
	};
}
