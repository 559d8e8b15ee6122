"""The cases of tests/chain_wrap_cases.py without a GPU (tests/test_gpu_chain_wraps.py runs them on the device).

* every block sequence is long enough to wrap the longest ring of its models twice and still run a block behind the second wrap;
* every case lands, at every block length of its sequence, on the chain instantiation it names (NA_DebugWaveNetKernel followed by
  NA_DebugWaveNetLaunch on 256 CUs), every other block length on the stage interpreter;
* together the cases reach every chain instantiation the launch switches hold, with every member set its family is run with, in a
  sequence of one block length and in the mixed one -- an uncovered one fails the test by name, and so does a deleted case;
* the table-launch cases land on the table instantiations they name;
* the oracle tells a long tap that is one frame off from the true one by more than 100 x the bound the GPU test applies."""
import numpy as np
import pytest

import chain_wrap_cases as CW
import na_oracle as O

CASES = CW.cases()
MODELS = ("standard", "lite", "feather", "nano", "a2")
CONTROL_MODELS = [("standard", 1.0), ("lite", 1.0), ("feather", 1.0), ("nano", 1.0), ("a2", 0.0), ("a2", 1.0)]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    loader = na.NeuralModelLoader()
    handles = {m: CW.load(loader, m) for m in MODELS}
    assert all(h is not None for h in handles.values())
    handles["loader"] = loader  # (the handles belong to it)
    return handles


def test_the_case_table_is_well_formed():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert len(set(CW.INSTANTIATIONS)) == len(CW.INSTANTIATIONS) == 25
    for case in CASES:
        assert sum(CW.SEQUENCES[case["seq"]]) == 2816 or case["seq"] == "mixed"
        assert all(count >= 1 for _, _, count in case["batch"])
        streams = [s for s, _, _ in CW.picks(case)]
        assert len(set(streams)) == len(streams) and all(0 <= s < CW.num_streams(case) for s in streams)
        assert case["expect"] or (case["seq"] == "mixed")
    assert sum(CW.SEQUENCES["mixed"]) == 4 * 810
    for seq in CW.SEQUENCES:
        x = CW.base_rows(seq)
        assert x.shape == (CW.BASE_ROWS, sum(CW.SEQUENCES[seq])) and x.dtype == np.float32 and np.array_equal(x, CW.base_rows(seq))
        assert np.abs(x).max() <= 1.0 and O.rms(x) > 0.25


def test_every_sequence_runs_a_block_behind_the_second_wrap_of_the_longest_ring():
    rings = {(m, q): CW.longest_ring(CW.oracle(m, q).arrays) for m, q in CONTROL_MODELS}
    assert rings == {("standard", 1.0): 1152, ("lite", 1.0): 1152, ("feather", 1.0): 1152, ("nano", 1.0): 1152, ("a2", 0.0): 1328, ("a2", 1.0): 1328}
    for case in CASES:
        total = sum(CW.SEQUENCES[case["seq"]])
        for model, quality, _ in case["batch"]:
            ring = CW.longest_ring(CW.oracle(model, quality).arrays)
            assert total >= 2 * ring + CW.BLOCK, (case["name"], model, total, ring)
            assert total - CW.LATE >= ring, (case["name"], model)  # the late window lies behind the first wrap of every ring


def test_every_case_lands_on_the_instantiation_it_names(na, models):
    wrong = []
    for case in CASES:
        for n in sorted(set(CW.SEQUENCES[case["seq"]])):
            got = CW.predict(na, models, case["batch"], n, knobs=case["knobs"])
            if n in case["expect"]:
                want = (CW.K_CHAIN,) + case["expect"][n] + (0,)
                assert n in CW.CHAIN_LENGTHS
            else:  # (no chain takes the length: 37, 100 and 1 frames, and 32 frames of A2)
                want = (CW.K_INTERPRETER,) + got[1:]
                assert n not in CW.CHAIN_LENGTHS or (n == 32 and case["expect"][128][0] == CW.CH_A2)
            if got != want:
                wrong.append((case["name"], n, got, want))
    assert not wrong, wrong


@pytest.fixture(scope="module")
def reached_by_case(na, models):
    """per case, the (instantiation, members, pure | mixed) its launches are predicted on"""
    out = []
    for case in CASES:
        groups = CW.launch_groups(na, models, case["batch"], case["knobs"])
        keys = set()
        for n in sorted(set(CW.SEQUENCES[case["seq"]])):
            got = CW.predict(na, models, case["batch"], n, knobs=case["knobs"])
            if got[0] == CW.K_CHAIN and got[5] == 0:
                keys.add((got[1:5], CW.signature(groups), "mixed" if case["seq"] == "mixed" else "pure"))
        out.append(keys)
    return out


def _uncovered(reached):
    return ["%s with members %s in a %s sequence" % (CW.instantiation_name(inst), sig, kind) for inst, sig, kind in CW.REQUIRED if (inst, sig, kind) not in reached]


def test_the_cases_reach_every_chain_instantiation_and_nothing_else(reached_by_case):
    """The union of the predictions is the explicit list, written from the switches; what is missing is named."""
    reached = set().union(*reached_by_case)
    missing = _uncovered(reached)
    assert not missing, "no case reaches " + "; ".join(missing)
    assert {k[0] for k in reached} == set(CW.INSTANTIATIONS), sorted({k[0] for k in reached} ^ set(CW.INSTANTIATIONS))
    assert set(reached) == set(CW.REQUIRED), sorted(set(reached) ^ set(CW.REQUIRED))
    assert {inst for inst, _, _ in CW.REQUIRED} == set(CW.INSTANTIATIONS)


def test_deleting_any_case_leaves_an_instantiation_uncovered(reached_by_case):
    for i, case in enumerate(CASES):
        missing = _uncovered(set().union(*(reached_by_case[:i] + reached_by_case[i + 1:])))
        assert missing and all("WaveNetSpecKernel<Fam" in m for m in missing), case["name"]


def test_the_table_cases_land_on_the_table_instantiations_they_name(na, models):
    """By stream count alone: nine handles of one file (a group each) at 128 and at 64 frames, both workgroup sizes of every family."""
    reached = set()
    for model, per, chain, spb, pk in CW.TABLE_CASES:
        groups = CW.table_groups(na, models[model], model, per)
        assert len(groups) == CW.TABLE_HANDLES > 8
        for seq in CW.TABLE_SEQUENCES:
            n = CW.SEQUENCES[seq][0]
            r = na.wavenet_launch(groups, n, cus=CW.CUS)
            assert (r[0], r[1], r[2], r[3], r[4], r[9]) == (CW.K_TABLE, 0, chain, n, spb, pk), (model, per, n, r)
            reached.add((chain, n, spb, pk))
    assert reached == {(c, n, s, pk) for c, pk in ((CW.CH_STD, 0), (CW.CH_LITE_PACKED, 1), (CW.CH_A2, 0)) for n in (128, 64) for s in (1, 2)}


@pytest.mark.parametrize("model,quality", CONTROL_MODELS, ids=["%s-%g" % m for m in CONTROL_MODELS])
def test_the_oracle_tells_a_long_tap_that_is_one_frame_off(model, quality):
    """Sensitivity control of the GPU test's late window: the same weights with the dilation of the layer of the longest reach lowered by
    one, on the rows the GPU test feeds, over the last 1024 frames -- more than 100 x TOL_RMS from the true oracle (measured 1.4e-3 ..
    6.1e-3 on signal_noise(2688, seed=7), 7 x .. 30 x the requirement).  Over the first 1024 frames of a prewarmed stream the same tap reads
    what the prewarm left."""
    ora = CW.oracle(model, quality)
    x = O.signal_noise(2688, seed=7)
    seven = O.rms(ora.process(x)[-CW.LATE:] - CW.off_by_one_oracle(ora).process(x)[-CW.LATE:])
    assert seven > CW.CONTROL_FACTOR * CW.TOL_RMS, (model, quality, seven)
    worst = seven
    for seq in CW.SEQUENCES:
        for row in CW.base_rows(seq)[:3]:
            apart = O.rms(CW.oracle(model, quality).process(row)[-CW.LATE:] - CW.off_by_one_oracle(ora).process(row)[-CW.LATE:])
            worst = min(worst, apart)
            assert apart > CW.CONTROL_FACTOR * CW.TOL_RMS, (model, quality, seq, apart)
    print("%s q = %g: one frame off is %.3g RMS over the late window on signal_noise(2688, 7), at least %.3g on the cases' rows; required %.3g" % (
        model, quality, seven, worst, CW.CONTROL_FACTOR * CW.TOL_RMS))
