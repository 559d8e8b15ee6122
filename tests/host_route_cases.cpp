// host_route_cases.cpp -- tests/test_host_route_cpu.py: the routing rule (neuralaudio_amd/csrc/host_route.h) over every combination of
// its facts.  The first line names the routes in enum order.  Then one line per combination of the eleven boolean facts (bit i of the
// first column, in the order of enum Fact below) and the unit counts 0 .. 3 (second column):
//   <bits> <units> | <blocking tries> <route: halves not prepared> <route: prepared> | <to-device route>
//                  | <submit tries> <route: not prepared> <route: prepared>
//                  | <device tries> <route: neither took it> <route: the resident launch took it> <route: the halves were prepared>
// A route function is asked about every outcome, also the ones its entry point never produces (an attempt it did not make).
#include <cstdio>

#include "host_route.h"

using namespace na;

static const char* const kRoutes[] = { "RegisteredInPlace", "StagedHalves", "StagedInPlace", "StagedCopies", "SubmitHalves", "SubmitInPlace",
	"SubmitOwnStream", "SubmitCopyStreams", "DeviceResident", "DeviceHalves", "DeviceOrdered", "ToDeviceInPlace", "ToDeviceCopies" };
static_assert(sizeof kRoutes / sizeof *kRoutes == (int)HostRoute::kCount, "a route without a name");

enum Fact { kHostDirect, kStageEntries, kResamples, kPinnedAddressable, kBothRegistered, kCallerPassedIn, kOtherTicketInFlight, kChainsInUse,
	kOwnsStream, kStreamObserved, kRowRangesOnly, kNumFacts };

int main()
{
	for (int r = 0; r < (int)HostRoute::kCount; r++) printf(r ? " %s" : "%s", kRoutes[r]);
	printf("\n");
	for (unsigned bits = 0; bits < (1u << kNumFacts); bits++)
		for (int units = 0; units <= 3; units++)
		{
			const auto is = [bits](Fact f) { return ((bits >> f) & 1u) != 0; };
			BlockingFacts b = {};
			b.hostDirect = is(kHostDirect);
			b.stageEntries = is(kStageEntries);
			b.bothRegistered = is(kBothRegistered);
			b.pinnedAddressable = is(kPinnedAddressable);
			b.rowRangesOnly = is(kRowRangesOnly);
			ToDeviceFacts t = {};
			t.hostDirect = is(kHostDirect);
			t.pinnedAddressable = is(kPinnedAddressable);
			SubmitFacts s = {};
			s.hostDirect = is(kHostDirect);
			s.stageEntries = is(kStageEntries);
			s.resamples = is(kResamples);
			s.pinnedAddressable = is(kPinnedAddressable);
			s.callerPassedIn = is(kCallerPassedIn);
			s.otherTicketInFlight = is(kOtherTicketInFlight);
			s.chainsInUse = is(kChainsInUse);
			s.launchUnits = units;
			DeviceFacts d = {};
			d.ownsStream = is(kOwnsStream);
			d.streamObserved = is(kStreamObserved);
			d.resamples = is(kResamples);
			d.stageEntries = is(kStageEntries);
			printf("%u %d | %d %s %s | %s | %d %s %s | %d %s %s %s\n", bits, units,
				(int)BlockingTriesHalves(b), kRoutes[(int)BlockingRouteFor(b, false)], kRoutes[(int)BlockingRouteFor(b, true)],
				kRoutes[(int)ToDeviceRouteFor(t)],
				(int)SubmitTriesHalves(s), kRoutes[(int)SubmitRouteFor(s, false)], kRoutes[(int)SubmitRouteFor(s, true)],
				(int)DeviceTriesFreeRunning(d), kRoutes[(int)DeviceRouteFor(d, false, false)], kRoutes[(int)DeviceRouteFor(d, true, false)],
				kRoutes[(int)DeviceRouteFor(d, false, true)]);
		}
	return 0;
}
