"""Both WaveNet kernel families -- and every kernel variant that ships behind a tuning knob -- against the oracle on EVERY architecture.

By default a model runs on the family that is faster for it (WaveNetKernelFor() in wavenet_choice.h: the f16-split kernel for Standard-like
models and padded A1 Lite, the f32 frame kernel for narrow / large-kernel ones, the runtime-shaped kernel for arrays wider than 16
channels; large batches of narrow models run packed).
NA_WN_KERNEL forces one family for all models it can run; it is read
once per process, so each forced run is a subprocess.  Two tiers: four fallbacks over the direct parity file ride in `-m gpu`
(seconds each); the full knob matrix over parity + fuzz + batch (245 tests per run) is a soak test behind `-m gpu_soak`.
Every subprocess has its own limit below the per-test watchdog, so a stall is reported with the output it produced."""
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = os.path.join(ROOT, "tests")
KNOBS = ("NA_WN_KERNEL", "NA_LSTM_NO_DPP", "NA_LSTM_LANE_KERNEL", "NA_REC_NOSKEW", "NA_WN_PACK", "NA_LSTM_NO_WAVE_RT", "NA_WN_SPEC", "NA_HOST_DIRECT",
         "NA_REC_QUAD_MIN", "NA_HOST_HALVES", "NA_REC_RPL", "NA_WN_DENSE", "NA_BATCH_NO_GRAPH", "NA_REC_NOPIPE", "NA_REC_L2W")

SOAK = [{"NA_WN_SPEC": "0"}, {"NA_WN_KERNEL": "split"}, {"NA_WN_KERNEL": "split", "NA_SP_T": "4"}, {"NA_WN_KERNEL": "split", "NA_SP_GEN": "1"},
        {"NA_WN_KERNEL": "frame"}, {"NA_WN_KERNEL": "frame", "NA_FR_PF": "2"}, {"NA_WN_KERNEL": "frame", "NA_FR_PF": "0"},
        {"NA_WN_KERNEL": "frame", "NA_FR_SPB": "4"}, {"NA_WN_KERNEL": "generic"}, {"NA_WN_PACK": "1"}, {"NA_LSTM_NO_DPP": "1", "NA_GRU_NO_DPP": "1"},
        {"NA_LSTM_LANE_KERNEL": "1"}, {"NA_REC_NOSKEW": "1", "NA_REC_NO_DPP32": "1"}, {"NA_LSTM_NO_WAVE_RT": "1"},
        {"NA_HOST_DIRECT": "0"},    # host buffers through the copy engines instead of kernels on the pinned block
        {"NA_REC_QUAD_MIN": "1"},   # every recurrent launch that can on the four-streams-per-wave layout, whatever its size
        {"NA_HOST_HALVES": "0"},    # no free-running half-batch chains: every buffer as ordered launches on the batch stream
        {"NA_WN_DENSE": "0"},       # four Nano streams at 16 / 16 virtual channels (default: 16 / 8, two streams per channel group)
        {"NA_REC_RPL": "4"},        # runtime-shaped recurrent kernel: four gate rows per lane (a quarter of the waves per stream)
        {"NA_BATCH_NO_GRAPH": "1"}, # multi-unit batches: fork / join issued directly every buffer (the path of a runtime older than the build's)
        {"NA_REC_L2W": "1"},        # runtime-shaped recurrent kernel: gate weights streamed from L2 also where they fit the LDS
        {"NA_REC_NOPIPE": "1"}]     # two-layer 16-unit LSTMs on one wave per stream (default: one wave per layer below 1536 waves)

# the four fallbacks a deployment can actually land on, over the direct parity file only: part of -m gpu, a few seconds each
SHORT = [{"NA_WN_KERNEL": "frame"}, {"NA_WN_SPEC": "0"}, {"NA_LSTM_NO_DPP": "1", "NA_GRU_NO_DPP": "1"}, {"NA_HOST_HALVES": "0"}]


def ident(e):
    return ",".join("%s=%s" % kv for kv in e.items())


def forced_run(env, files, limit):
    if any(os.environ.get(k) for k in KNOBS):
        pytest.skip("already inside a forced run")
    e = dict(os.environ, **env)
    t0 = time.monotonic()
    try:    # --durations: a slow forced run names its slow tests in the failure text
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--durations=8", "-p", "no:cacheprovider"] + files,
                           env=e, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as ex:
        out = ex.stdout.decode(errors="replace") if isinstance(ex.stdout, bytes) else (ex.stdout or "")
        pytest.fail("forced run %s did not finish in %d s; output so far:\n%s" % (ident(env), limit, out[-3000:]))
    assert r.returncode == 0, "%.0f s\n" % (time.monotonic() - t0) + r.stdout[-3000:] + r.stderr[-1500:]


@pytest.mark.gpu
@pytest.mark.watchdog(260)
@pytest.mark.parametrize("env", SHORT, ids=ident)
def test_forced_fallback_passes_the_parity_suite(env):
    # (the parity file needs no torch: the child skips the warm import -- 16 s on a good box; one r06 run on a box with slow storage
    # spent more than 100 s before the child's first test, hence the generous limit)
    forced_run(dict(env, NA_TEST_NO_WARM="1"), [os.path.join(T, "test_gpu_parity.py")], 240)


# the runtime-shaped recurrent kernel's two forced regimes over its own file: every shape on L2-streamed weights (also the one-wave
# shapes whose weights fit the LDS), and eight gate rows per lane (LSTMs of 600-odd, 769 and 1024 units reach dispatch cases 5, 7 and 8).
# The regime assertions of that file skip under a knob; the parity assertions do not.
RECURRENT_RT = [{"NA_REC_L2W": "1"}, {"NA_REC_RPL": "8"}]


@pytest.mark.gpu
@pytest.mark.watchdog(260)
@pytest.mark.parametrize("env", RECURRENT_RT, ids=ident)
def test_forced_recurrent_regime_passes_the_runtime_shaped_kernel_suite(env):
    forced_run(dict(env, NA_TEST_NO_WARM="1"), [os.path.join(T, "test_gpu_recurrent_rt.py")], 240)


# the keras-stack tails over their own file: the lane = stream kernels' DenseTail calls (LstmGenericKernel / GruGenericKernel: 64 streams per
# workgroup, idle lanes in the last one) under the two knobs that send dense-tail models there, and the runtime-shaped kernel on
# L2-streamed weights in front of both tail forms.  Conv1d tails stay on the runtime-shaped kernel under all three; a dense-tail case beyond
# the lane = stream kernels' LDS bound skips under the first two.  (The file's in-place tests import torch: the child keeps the warm import.)
TAILS = [{"NA_LSTM_NO_WAVE_RT": "1"}, {"NA_LSTM_LANE_KERNEL": "1"}, {"NA_REC_L2W": "1"}]


@pytest.mark.gpu
@pytest.mark.watchdog(260)
@pytest.mark.parametrize("env", TAILS, ids=ident)
def test_forced_recurrent_kernel_passes_the_tail_suite(env):
    forced_run(env, [os.path.join(T, "test_gpu_tails.py")], 240)


# the f32 frame kernel's instantiations that ship behind a tuning knob over its own file (the knobs do not skip it): ring history
# prefetched into LDS (Launch<2, 2, 1> and <2, 2, 2>), no prefetch at all for long buffers too (<2, 0, 1>), and four streams per workgroup
# (<2, 1, 4>) -- each takes the default shape where its LDS does not fit (frame_lds.h), which the file's large-kernel tests reach.
FRAME = [{"NA_FR_PF": "2"}, {"NA_FR_PF": "0"}, {"NA_FR_SPB": "4"}]


@pytest.mark.gpu
@pytest.mark.watchdog(260)
@pytest.mark.parametrize("env", FRAME, ids=ident)
def test_forced_frame_kernel_regime_passes_the_frame_kernel_suite(env):
    forced_run(dict(env, NA_TEST_NO_WARM="1"), [os.path.join(T, "test_gpu_frame.py")], 240)


@pytest.mark.gpu_soak
@pytest.mark.watchdog(330)
@pytest.mark.parametrize("env", SOAK, ids=ident)
def test_forced_family_passes_parity_fuzz_and_batch_suites(env):
    forced_run(env, [os.path.join(T, "test_gpu_parity.py"), os.path.join(T, "test_gpu_fuzz.py"), os.path.join(T, "test_gpu_batch.py")], 300)


# Multi-unit batches (a buffer of several launches on forked side streams): the suite runs on the runtime the library was built for, which
# replays a captured hipGraph; NA_BATCH_NO_GRAPH issues the fork / join directly every buffer -- the path of an older runtime
# (NA_TEST_TORCH_FIRST) -- over the tests that process such batches.  They import torch: the child keeps the warm import.
DIRECT_FORK_JOIN = ["test_gpu_batch.py::test_config4_lstm_2x16_many_streams_and_mixed_with_wavenet",
                    "test_gpu_batch.py::test_table_launches_inside_a_captured_multi_unit_batch_replay_their_own_tables",
                    "test_gpu_recurrent_quad.py::test_four_streams_per_wave_kernel_is_right_beside_matrix_waves_of_another_kernel"]


@pytest.mark.gpu
@pytest.mark.watchdog(260)
def test_multi_unit_batches_pass_with_the_fork_join_issued_directly():
    forced_run({"NA_BATCH_NO_GRAPH": "1"}, [os.path.join(T, t) for t in DIRECT_FORK_JOIN], 240)
