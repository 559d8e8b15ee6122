"""Which model groups of a batch share a launch (neuralaudio_amd/csrc/launch_plan.h), host side only: the planner against a restatement
of the rules it replaced -- the sort of a mixed batch's groups into fused launch lists in GpuBatch::ProcessDeviceOn, the unit count of
GpuBatch::LaunchUnitsAfterSwitch, and the conditions of GpuBatch::PrepareHalves (free-running chains) and GpuBatch::ResidentConfigure
(the resident launch) -- over every sequence of group kinds up to four groups, and over longer runs for the eight-group limit.

The restatement speaks the integer codes of the old ModelGroup::LaunchClass(): 0 frame kernel, 1 f16-split kernel, 2 f16-split kernel
with packed streams, -1 f16-split kernel that joins the packed launch when the batch has one (else the split launch), 3 the fused
LDS-free recurrent launch, -2 a launch of its own."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"Frame": 0, "Split": 1, "SplitJoinsPacked": -1, "SplitPacked": 2, "Recurrent": 3, "Own": -2}
LIST_NAME = {0: "Frame", 1: "Split", 2: "SplitPacked"}
MAX_GROUPS = 8  # WN_FRAME_MAX_GROUPS


def old_units(codes):
    """ProcessDeviceOn's sort: the three WaveNet lists, the joiners resolved after all groups were seen (behind each list's own groups),
    the recurrent list, the singles; a list's first group lends the unit its side stream."""
    fused, joiners, rec, singles = {0: [], 1: [], 2: []}, [], [], []
    for i, c in enumerate(codes):
        if c in fused:
            fused[c].append(i)
        elif c == -1:
            joiners.append(i)
        elif c == 3:
            rec.append(i)
        else:
            singles.append(i)
    for j in joiners:
        fused[1 if not fused[2] else 2].append(j)
    units = [(LIST_NAME[l], fused[l]) for l in (0, 1, 2) if fused[l]]
    if rec:
        units.append(("Recurrent", rec))
    return units + [("Own", [s]) for s in singles]


def old_unit_count(codes):
    """LaunchUnitsAfterSwitch: its own copy of the joiner rule."""
    lists, joiner, rec, singles = [False] * 3, False, False, 0
    for c in codes:
        if 0 <= c <= 2:
            lists[c] = True
        elif c == -1:
            joiner = True
        elif c == 3:
            rec = True
        else:
            singles += 1
    if joiner and not lists[2]:
        lists[1] = True
    return sum(lists) + int(rec) + singles


def old_halves(codes):
    """PrepareHalves before its stream count: split kernels only, not plain and packed together, 1 .. 8 groups."""
    if any(c not in (1, 2, -1) for c in codes):
        return False
    return 0 < len(codes) <= MAX_GROUPS and not (2 in codes and 1 in codes)


def old_resident(codes):
    """ResidentConfigure before its architecture and stream counts: the plain split launch only, 1 .. 8 groups."""
    return all(c in (1, -1) for c in codes) and 0 < len(codes) <= MAX_GROUPS


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_plan") / "launch_plan_cases"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "launch_plan_cases.cpp"), "-o", str(exe)], check=True)

    def plan(sequences):
        text = "".join(" ".join(s) + "\n" for s in sequences)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(sequences)
        result = []
        for line in out:
            units_text, flags = line.split("|")
            units = [(u.split(":")[0], [int(i) for i in u.split(":")[1].split(",")]) for u in units_text.split()]
            halves, resident = (bool(int(f)) for f in flags.split())
            result.append((units, halves, resident))
        return result

    return plan


def check(planner, sequences):
    for seq, (units, halves, resident) in zip(sequences, planner(sequences)):
        codes = [CODE[k] for k in seq]
        assert units == old_units(codes), seq
        assert len(units) == old_unit_count(codes), seq
        assert halves == old_halves(codes), seq
        assert resident == old_resident(codes), seq


def test_every_mix_of_up_to_four_groups_plans_the_launches_of_the_old_rules(planner):
    sequences = [s for n in range(5) for s in itertools.product(sorted(CODE), repeat=n)]
    assert len(sequences) == 1555
    check(planner, sequences)
    # the example of the issue that moved the rule here: a joiner beside a plain and a packed group rides in the packed launch -- two
    # units, so no free-running chains
    assert planner([("Split", "SplitPacked", "SplitJoinsPacked")])[0] == ([("Split", [0]), ("SplitPacked", [1, 2])], False, False)


def test_the_chains_and_the_resident_launch_take_at_most_eight_groups(planner):
    runs = [(k,) * n for k in ("Split", "SplitJoinsPacked", "SplitPacked") for n in (7, 8, 9, 12)]
    runs += [("SplitPacked",) * (n - 1) + ("SplitJoinsPacked",) for n in (8, 9)]
    runs += [("SplitJoinsPacked",) * (n - 1) + ("Split",) for n in (8, 9)]
    check(planner, runs)
