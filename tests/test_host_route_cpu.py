"""How a buffer is routed onto the device (neuralaudio_amd/csrc/host_route.h), host side only: the rule against a restatement of the
nested conditions it replaced in the four processing entry points of GpuBatch -- ProcessHost, ProcessHostToDevice, Submit and
ProcessDevice -- over every combination of its facts: eleven booleans and the unit counts 0 .. 3.

The restatement keeps the shape of the old code: an attempt at the free-running forms (PrepareHalves, TryResident) had side effects and
was only made where the conditions in front of it held, so each old_* function returns whether the attempt was made beside the route,
and reads the attempt's outcome only where the old code made it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTS = ("hostDirect", "stageEntries", "resamples", "pinnedAddressable", "bothRegistered", "callerPassedIn", "otherTicketInFlight",
         "chainsInUse", "ownsStream", "streamObserved", "rowRangesOnly")  # bit order of host_route_cases.cpp


def old_process_host(f, prepared):
    if f["hostDirect"]:
        if f["bothRegistered"] and not f["stageEntries"]:
            return False, "RegisteredInPlace"
    direct = f["hostDirect"] and not f["stageEntries"] and f["pinnedAddressable"]
    if direct and prepared and f["rowRangesOnly"]:  # (direct && PrepareHalves(n) && halfLists->RowRangesOnly())
        return True, "StagedHalves"
    return direct, "StagedInPlace" if direct else "StagedCopies"


def old_process_host_to_device(f):
    return "ToDeviceInPlace" if f["hostDirect"] and f["pinnedAddressable"] else "ToDeviceCopies"


def old_submit(f, units, prepared):
    direct = f["hostDirect"] and not f["stageEntries"]
    if direct and f["pinnedAddressable"]:
        tried = not f["callerPassedIn"] and (f["otherTicketInFlight"] or f["chainsInUse"])
        if tried and prepared:
            return True, "SubmitHalves"
        return tried, "SubmitInPlace"
    if units <= 1 and not f["resamples"]:
        return False, "SubmitOwnStream"
    return False, "SubmitCopyStreams"


def old_process_device(f, resident, prepared):
    runs_ordered = f["resamples"] or f["stageEntries"]
    if f["ownsStream"] and not f["streamObserved"] and not runs_ordered:
        if resident:
            return True, "DeviceResident"
        if prepared:
            return True, "DeviceHalves"
        return True, "DeviceOrdered"
    return False, "DeviceOrdered"


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_route") / "host_route_cases"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_route_cases.cpp"), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    return lines[0].split(), [[part.split() for part in line.split("|")] for line in lines[1:]]


def test_the_rule_routes_every_combination_of_facts_as_the_old_conditions_did(grid):
    names, rows = grid
    assert len(rows) == (1 << len(FACTS)) * 4
    seen = set()
    for (bits, units), blocking, to_device, submit, device in rows:
        f = {name: bool((int(bits) >> i) & 1) for i, name in enumerate(FACTS)}
        units, where = int(units), (bits, units)
        for k, prepared in enumerate((False, True)):
            tried, route = old_process_host(f, prepared)
            assert (bool(int(blocking[0])), blocking[1 + k]) == (tried, route), where
            tried, route = old_submit(f, units, prepared)
            assert (bool(int(submit[0])), submit[1 + k]) == (tried, route), where
        assert to_device == [old_process_host_to_device(f)], where
        for k, (resident, prepared) in enumerate(((False, False), (True, False), (False, True))):
            tried, route = old_process_device(f, resident, prepared)
            assert (bool(int(device[0])), device[1 + k]) == (tried, route), where
        # an outcome is only real where the attempt was made
        seen.update([blocking[1], to_device[0], submit[1], device[1]])
        seen.update([blocking[2]] if int(blocking[0]) else [])
        seen.update([submit[2]] if int(submit[0]) else [])
        seen.update(device[2:] if int(device[0]) else [])
    assert seen == set(names), "a route no combination of facts reaches"


def test_the_package_names_the_routes_in_the_order_of_the_enum(grid):
    import neuralaudio_amd
    assert list(neuralaudio_amd.HOST_ROUTES) == grid[0]
