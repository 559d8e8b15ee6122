"""Every compiled WaveNet chain instantiation, in batches, past its ring wraps (tests/chain_wrap_cases.py; tests/test_chain_wraps_cpu.py
proves without a GPU that the cases land where they say and reach every instantiation of the launch switches).

The runs of tests/test_gpu_spec.py are 256 .. 810 frames long: no long tap of theirs reads a frame the kernel stored itself, and no exact
ring wraps.  Here every case runs 2816 frames or more -- [128] x 22, [64] x 44, [32] x 88, and a mixed sequence that hands the state
between chain and interpreter on both sides of the wraps -- on ONE launch per block (ProcessDevice on the caller's stream: a host-buffer
call of 512 streams or more would run as two half-batch launches at the smaller workgroup size), twice: with the chains on and with the
stage interpreter alone.  Per case:

* the library predicts, for this device's CU count and this batch's state size, the instantiation the case names (skipped where the
  process runs under launch knobs of its own);
* chain and interpreter agree bit for bit over the whole run, all streams; streams of one model fed the same row carry the same bits;
* the first, a middle and the last stream of every AddStreams call are within TOL_RMS = 2e-6 of the C oracle, over the whole run and
  over the last 1024 frames alone, where every long tap reads self-stored frames behind a wrap.

The one-tile-per-wave chain takes 16 / 16 packs, which exist under NA_WN_DENSE=0 only, and the non-temporal variants of the lite and A2
families need more state than these batches hold unless NA_WN_NT_MB lowers the threshold: the tuning knobs are read once per process, so
both run in a fresh child process (this file with --child), which writes its outputs to a file the parent judges."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_wrap_cases as CW
import na_oracle as O

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

TOL_RMS = CW.TOL_RMS
CASES = CW.cases()
HERE = [c for c in CASES if not c["knobs"]]
DENSE_OFF = [c for c in CASES if c["knobs"]]
NT_CASES = ["lite-513-128", "feather-1029-128", "nano-2057-128", "a2-810-128"]  # the SPB = 2 launches of 128 frames of the other families
MODELS = ("standard", "lite", "feather", "nano", "a2")
DEVICE_ORDERED = "DeviceOrdered"


def _own_launch_knobs(but=()):
    return sorted(k for k in os.environ if k.startswith(("NA_SP_", "NA_WN_", "NA_HOST_", "NA_RESIDENT")) and k not in but)


# ---- running a case (parent and child) ------------------------------------------------------------------------------------------------
def load_models(na):
    loader = na.NeuralModelLoader()
    handles = {m: CW.load(loader, m) for m in MODELS}
    assert all(h is not None for h in handles.values())
    handles["loader"] = loader
    return handles


def run_case(na, models, case, variants=(True, False)):
    """The case's batch over its sequence, once per variant (True: chains on, False: the stage interpreter alone).  Returns the outputs
    [streams, frames] per variant and what the batch said about itself."""
    import torch
    lib = na.capi.load_library()
    dev = torch.device("cuda", 0)
    sizes = CW.SEQUENCES[case["seq"]]
    total, streams = sum(sizes), CW.num_streams(case)
    ts = torch.cuda.Stream(device=dev)
    x = torch.from_numpy(CW.base_rows(case["seq"])).to(dev)[torch.arange(streams, device=dev) % CW.BASE_ROWS].contiguous()
    outs, meta = {}, dict(names={}, routes={}, predicted={})
    try:
        for on in variants:
            lib.NA_DebugSetWaveNetSpec(1 if on else 0)
            b = na.Batch(0, hip_stream=ts.cuda_stream)
            for model, quality, count in case["batch"]:
                b.AddStreams(models[model], count, quality=quality)
            assert b.NumStreams() == streams
            y = torch.zeros_like(x)
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(ts):
                at = 0
                for n in sizes:
                    b.ProcessDevice(x[:, at:].data_ptr(), y[:, at:].data_ptr(), n, total, total)
                    at += n
                b.Synchronize()
            key = "chain" if on else "interp"
            meta["names"][key] = sorted({b.StreamKernelName(s) for s, _, _ in CW.picks(case)})
            meta["routes"][key] = na.HOST_ROUTES[b.DebugLastHostRoute()]
            if on:
                # what the library decides for the launches this batch made: its own knobs, this device, this state size
                limit = int(os.environ.get("NA_WN_NT_MB") or 400) << 20
                meta["state_bytes"] = b.StateBytes()
                meta["beyond_cache"] = bool(os.environ.get("NA_WN_NT") != "0" and meta["state_bytes"] > limit)
                meta["cus"] = int(torch.cuda.get_device_properties(0).multi_processor_count)
                for n in sorted(set(sizes)):
                    meta["predicted"][str(n)] = list(CW.predict(na, models, case["batch"], n, cus=meta["cus"], beyond_cache=meta["beyond_cache"], knobs=None))
            outs[key] = y.cpu().numpy()
            b.close()
    finally:
        lib.NA_DebugSetWaveNetSpec(1)
    return outs, meta


def child_main(argv):
    """--child OUT.npz both|chain CASE...: the cases under this process's knobs"""
    sys.path[:0] = [O.ROOT, os.path.join(O.ROOT, "tests")]
    import neuralaudio_amd as na
    out_path, variants, names = argv[0], (True, False) if argv[1] == "both" else (True,), argv[2:]
    models = load_models(na)
    arrays = {}
    for name in names:
        outs, meta = run_case(na, models, CW.by_name(name), variants)
        for key, y in outs.items():
            arrays["%s/%s" % (name, key)] = y
        arrays["%s/meta" % name] = np.array(json.dumps(meta))
    np.savez(out_path, **arrays)
    print("CHILD DONE %d" % len(names))


def _child(tmp_path, knobs, variants, names):
    """one fresh process (never an exec of this one) under `knobs`; returns {case: (outs, meta)}"""
    out_path = tmp_path / "chain_wraps_child.npz"
    env = dict(os.environ, **{k: str(v) for k, v in knobs.items()})
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(out_path), variants] + list(names), env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as ex:
        pytest.fail("the child under %s did not finish in 240 s: %s" % (knobs, (ex.stdout or b"")[-2000:]))
    assert r.returncode == 0 and "CHILD DONE %d" % len(names) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out_path)
    return {name: ({key: got["%s/%s" % (name, key)] for key in ("chain", "interp") if "%s/%s" % (name, key) in got.files},
                   json.loads(str(got["%s/meta" % name]))) for name in names}


# ---- judging a case -------------------------------------------------------------------------------------------------------------------
_ORACLE = {}     # (model, submodel, sequence, row) -> the oracle's output: computed once per module, never written to
_CHAIN_OUT = {}  # the chain outputs of NT_CASES in this (ordinary) process, for the non-temporal test


def _oracle_row(model, quality, seq, row):
    key = (model, CW.submodel(model, quality), seq, row)
    if key not in _ORACLE:
        y = CW.oracle(model, quality).process(CW.base_rows(seq)[row])
        y.setflags(write=False)
        _ORACLE[key] = y
    return _ORACLE[key]


def judge(case, outs, meta, own_knobs):
    name = case["name"]
    chain, interp = outs["chain"], outs["interp"]
    assert meta["routes"] == {"chain": DEVICE_ORDERED, "interp": DEVICE_ORDERED}, (name, meta["routes"])  # one launch of all the groups per block
    assert meta["names"] == {"chain": ["WaveNetSpecKernel"], "interp": ["WaveNetSplitKernel"]}, (name, meta["names"])
    if not own_knobs:
        for n, inst in case["expect"].items():
            assert tuple(meta["predicted"][str(n)]) == (CW.K_CHAIN,) + inst + (0,), (name, n, meta["predicted"], meta["cus"], meta["state_bytes"])
        for n in set(CW.SEQUENCES[case["seq"]]) - set(case["expect"]):
            assert meta["predicted"][str(n)][0] == CW.K_INTERPRETER, (name, n, meta["predicted"])
    assert chain.shape == (CW.num_streams(case), sum(CW.SEQUENCES[case["seq"]])) and np.all(np.isfinite(chain))
    if not np.array_equal(chain, interp):
        bad = np.argwhere(chain != interp)
        pytest.fail("%s: chain and interpreter differ in %d values of %d streams, first at stream %d frame %d, largest %.3g" % (
            name, len(bad), len(set(bad[:, 0])), bad[0][0], bad[:, 1].min(), float(np.abs(chain - interp).max())))
    for model, quality, first, count in CW.group_ranges(case):
        rows = (first + np.arange(count)) % CW.BASE_ROWS
        for row in set(rows.tolist()):
            same = first + np.flatnonzero(rows == row)
            assert np.all(chain[same] == chain[same[0]]), (name, model, quality, row)
    worst = [0.0, 0.0]
    for s, model, quality in CW.picks(case):
        yo = _oracle_row(model, quality, case["seq"], s % CW.BASE_ROWS)
        whole, late = O.rms(chain[s] - yo), O.rms(chain[s][-CW.LATE:] - yo[-CW.LATE:])
        worst = [max(worst[0], whole), max(worst[1], late)]
        assert whole < TOL_RMS and late < TOL_RMS, (name, s, model, quality, whole, late)
    print("chain-wrap-error %-24s chain - oracle RMS: whole run %.3g, last %d frames %.3g (bound %.3g)" % (name, worst[0], CW.LATE, worst[1], TOL_RMS))


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    return load_models(na)


@pytest.fixture()
def spec_switch(na):
    yield
    na.capi.load_library().NA_DebugSetWaveNetSpec(1)


@pytest.mark.parametrize("case", HERE, ids=[c["name"] for c in HERE])
def test_chain_is_bit_identical_to_the_interpreter_and_on_the_oracle_behind_the_wraps(na, models, spec_switch, case):
    outs, meta = run_case(na, models, case)
    if case["name"] in NT_CASES:
        _CHAIN_OUT[case["name"]] = outs["chain"]
    judge(case, outs, meta, _own_launch_knobs())


@pytest.fixture(scope="module")
def dense_off_runs(tmp_path_factory):
    """all cases of the 16 / 16 pack in ONE child under NA_WN_DENSE=0"""
    knobs = DENSE_OFF[0]["knobs"]
    assert all(c["knobs"] == knobs for c in DENSE_OFF)
    return _child(tmp_path_factory.mktemp("dense_off"), knobs, "both", [c["name"] for c in DENSE_OFF])


@pytest.mark.watchdog(260)
@pytest.mark.parametrize("case", DENSE_OFF, ids=[c["name"] for c in DENSE_OFF])
def test_one_tile_chain_of_the_16_16_pack_in_a_process_of_its_own(dense_off_runs, case):
    outs, meta = dense_off_runs[case["name"]]
    judge(case, outs, meta, _own_launch_knobs(but=case["knobs"]))


@pytest.mark.watchdog(260)
def test_non_temporal_variants_of_the_other_families_compute_the_same_bits_behind_the_wraps(na, models, spec_switch, tmp_path):
    """Cfg::NT marks the ring traffic of the long dilations non-temporal: a cache-policy bit.  A child under NA_WN_NT_MB=1 runs the
    SPB = 2 cases of Lite, Feather, Nano and A2 over [128] x 22 on the NT bodies; the ordinary bodies of this process must have computed
    the same bits (and are held to the interpreter and the oracle by the test above)."""
    cases = [CW.by_name(n) for n in NT_CASES]
    assert all(c["expect"][128][2] == 2 for c in cases)
    theirs = _child(tmp_path, {"NA_WN_NT_MB": 1}, "chain", NT_CASES)
    own_knobs = _own_launch_knobs()
    for case in cases:
        name = case["name"]
        if name not in _CHAIN_OUT:
            outs, meta = run_case(na, models, case, (True,))
            assert not meta["beyond_cache"] or own_knobs, (name, meta)
            _CHAIN_OUT[name] = outs["chain"]
        outs, meta = theirs[name]
        assert meta["routes"]["chain"] == DEVICE_ORDERED and meta["names"]["chain"] == ["WaveNetSpecKernel"], (name, meta)
        if not own_knobs:
            assert meta["beyond_cache"] and tuple(meta["predicted"]["128"]) == (CW.K_CHAIN,) + case["expect"][128] + (1,), (name, meta)
        assert np.array_equal(outs["chain"], _CHAIN_OUT[name]), (name, float(np.abs(outs["chain"] - _CHAIN_OUT[name]).max()))
    _CHAIN_OUT.clear()


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child_main(sys.argv[2:])
