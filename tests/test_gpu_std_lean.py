"""The A1 Standard chain after its waves stopped issuing work their own frames do not need (wavenet_spec_impl.h Cfg::LEAN): still bit for bit
the stage interpreter, over runs long enough to wrap every ring.

* 20 blocks of 128 frames wrap the 1024-frame ring of the d = 512 layers twice and every compact ring many times (six blocks, as in
  test_gpu_spec.py, never read a stored frame through the -1024 tap and wrap no exact ring).
* A sequence that alternates 128-frame blocks with 37- and 100-frame ones hands the stream state from the chain to the interpreter and
  back in mid-stream.
* 3 streams: a partial last workgroup, whose shadow waves must stage weights and meet barriers like live ones.
"""
import os

import numpy as np
import pytest

import na_oracle as O

pytestmark = pytest.mark.gpu

TOL_RMS = 2e-6
FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
MODEL = "BossWN-standard.nam"
SEQUENCES = {"long": [128] * 20, "mixed": [128, 37, 128, 100, 128, 128, 37, 128, 100, 128, 128, 37, 128]}
BASE_STREAMS = 5


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def model(na):
    return na.NeuralModelLoader().CreateFromFile(os.path.join(O.MODELS_DIR, MODEL), doPrewarm=False)


@pytest.fixture()
def spec_switch(na):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    yield lambda on: lib.NA_DebugSetWaveNetSpec(1 if on else 0)
    lib.NA_DebugSetWaveNetSpec(1)


@pytest.fixture(scope="module")
def signals():
    """per sequence: the input rows and (computed once, never changed) the oracle's output of each row"""
    rng = np.random.default_rng(29)
    out = {}
    for name, sizes in SEQUENCES.items():
        x = (0.3 * rng.standard_normal((BASE_STREAMS, sum(sizes)))).clip(-1, 1).astype(np.float32)
        out[name] = (x, {})
    return out


def _oracle(signals, name, row):
    x, cache = signals[name]
    if row not in cache:
        cache[row] = O.oracle_from_file(MODEL).process(x[row])
    return cache[row]


def _run(batch, x, sizes):
    out, a = [], 0
    for c in sizes:
        out.append(batch.Process(np.ascontiguousarray(x[:, a:a + c])))
        a += c
    return np.concatenate(out, axis=1)


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("streams", [1, 2, 3, 5])
@pytest.mark.parametrize("seq", ["long", "mixed"])
def test_standard_chain_is_bit_identical_to_the_interpreter_across_ring_wraps(na, model, spec_switch, signals, seq, streams):
    sizes = SEQUENCES[seq]
    x = signals[seq][0][:streams]
    ys = []
    for on in (True, False):
        spec_switch(on)
        b = na.Batch(0)
        b.AddStreams(model, streams)
        assert b.StreamKernelName(0) == ("WaveNetSpecKernel" if on else "WaveNetSplitKernel")
        ys.append(_run(b, x, sizes))
        b.close()
    spec_switch(True)
    assert np.all(np.isfinite(ys[0]))
    assert np.array_equal(ys[0], ys[1]), (seq, streams, float(np.abs(ys[0] - ys[1]).max()))
    for s in sorted({0, streams - 1}):
        assert O.rms(ys[0][s] - _oracle(signals, seq, s)) < TOL_RMS, (seq, s)
