"""Host-side tests of the stream snapshots (csrc/stream_snapshot.h): sizes, fingerprint, refusals without a device, and
the pinned format of version 1.  No GPU needed.

The format reader below is pure Python on purpose: it is the second, independent description of format version 1.  A change of the
layout must bump kSnapshotVersion (and add a new golden blob), not edit this reader."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import na_oracle as O

GOLDEN_BLOB = os.path.join(O.ROOT, "tests", "golden", "snapshots", "lstm_1x16_v1.bin")
MAGIC = 0x5353414E  # "NASS"
FIXED_HEADER = 48
SECTION_ENTRY = 16
KIND_WAVENET, KIND_LSTM = 1, 2
ENC_F32, ENC_SPLIT = 0, 1


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def _load(na, name, **kw):
    loader = na.NeuralModelLoader()
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False, **kw)
    assert m is not None
    m._loader = loader
    return m


def parse_snapshot(blob):
    """format version 1 -> (header dict, [section dict with its payload words])"""
    magic, version, total, fingerprint, nsub, active, quality, flags, prewarmed, header_bytes = struct.unpack_from("<IIQQIIfIII", blob, 0)
    head = dict(magic=magic, version=version, total=total, fingerprint=fingerprint, nsub=nsub, active=active, quality=quality, flags=flags,
                prewarmed=prewarmed, header_bytes=header_bytes)
    sections = []
    for k in range(nsub):
        kind, enc, values, offset = struct.unpack_from("<IIII", blob, FIXED_HEADER + SECTION_ENTRY * k)
        sections.append(dict(kind=kind, encoding=enc, values=values, offset=offset,
                             words=np.frombuffer(blob, dtype="<u4", count=values, offset=offset)))
    return head, sections


def wavenet_values(layers):
    """values of a WaveNet section from a .nam 'layers' list: per conv layer (K - 1) d frames of `channels`, plus the conv head's ring"""
    n = 0
    for lc in layers:
        ks = lc["kernel_sizes"] if "kernel_sizes" in lc else [lc["kernel_size"]] * len(lc["dilations"])
        n += sum((int(k) - 1) * int(d) for k, d in zip(ks, lc["dilations"])) * int(lc["channels"])
        if "head" in lc and isinstance(lc["head"], dict) and int(lc["head"]["kernel_size"]) > 1:
            n += (int(lc["head"]["kernel_size"]) - 1) * int(lc["channels"])
    return n


@pytest.mark.parametrize("name,values", [("BossWN-standard.nam", 2 * 1023 * 16 + 2 * 1023 * 8), ("BossWN-nano.nam", 2 * 127 * 4 + 2 * 1919 * 2),
                                         ("BossLSTM-1x16.nam", 32)])
def test_known_answer_sizes(na, name, values):
    assert values in (49104, 8692, 32)
    m = _load(na, name)
    assert na.snapshot_bytes(m) == FIXED_HEADER + SECTION_ENTRY + 4 * values
    assert m.SnapshotBytes() == na.snapshot_bytes(m)


def test_slimmable_container_is_the_sum_of_its_submodels(na):
    j = O.load_json("BossWN-a2.nam")
    subs = j["config"]["submodels"]
    assert len(subs) == 2
    values = [wavenet_values(s["model"]["config"]["layers"]) for s in subs]
    assert all(v > 0 for v in values)
    for q in (0.0, 1.0):  # (the size does not depend on which submodel is active: inactive ones are frozen state too)
        loader = na.NeuralModelLoader()
        loader.SetDefaultQualityScaleFactor(q)
        m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-a2.nam"), doPrewarm=False)
        assert na.snapshot_bytes(m) == FIXED_HEADER + 2 * SECTION_ENTRY + 4 * sum(values)


def test_fingerprint(na):
    a, b = _load(na, "BossWN-standard.nam"), _load(na, "BossWN-standard.nam")
    fa = na.snapshot_fingerprint(a)
    assert fa != 0 and fa == na.snapshot_fingerprint(b)
    # two weight sets of one architecture
    arrays = O.a1_arrays(16, 8)
    loader = na.NeuralModelLoader()
    s1 = loader.CreateFromString(O.nam_json_wavenet_a1(16, 8, O.synth_wavenet_weights(arrays, seed=1)), ".nam", doPrewarm=False)
    s2 = loader.CreateFromString(O.nam_json_wavenet_a1(16, 8, O.synth_wavenet_weights(arrays, seed=2)), ".nam", doPrewarm=False)
    f1, f2 = na.snapshot_fingerprint(s1), na.snapshot_fingerprint(s2)
    assert f1 != f2 and fa not in (f1, f2)
    assert na.snapshot_bytes(s1) == na.snapshot_bytes(s2) == na.snapshot_bytes(a)
    # the math mode is no part of it
    std = na.NeuralModelLoader()
    std.SetWaveNetMathMode(na.EMathMode.StdMath)
    std.SetLSTMMathMode(na.EMathMode.StdMath)
    assert na.snapshot_fingerprint(std.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-standard.nam"), doPrewarm=False)) == fa
    lstm = _load(na, "BossLSTM-1x16.nam")
    assert na.snapshot_fingerprint(std.CreateFromFile(os.path.join(O.MODELS_DIR, "BossLSTM-1x16.nam"), doPrewarm=False)) == na.snapshot_fingerprint(lstm)
    assert na.snapshot_fingerprint(lstm) != fa


def test_fingerprint_does_not_depend_on_the_kernel_family_knobs(na, tmp_path):
    """NA_WN_KERNEL / NA_WN_PACK are read once per process: a child process per setting prints the fingerprint."""
    import subprocess
    import sys
    script = tmp_path / "fp.py"
    script.write_text("import os, sys\nsys.path.insert(0, %r)\nimport neuralaudio_amd as na\n"
                      "m = na.NeuralModelLoader().CreateFromFile(%r, doPrewarm=False)\nprint(na.snapshot_fingerprint(m), na.snapshot_bytes(m))\n"
                      % (O.ROOT, os.path.join(O.MODELS_DIR, "BossWN-nano.nam")))
    seen = set()
    for env in ({}, {"NA_WN_KERNEL": "frame"}, {"NA_WN_KERNEL": "split", "NA_WN_PACK": "0"}, {"NA_WN_DENSE": "0"}):
        e = {k: v for k, v in os.environ.items() if not k.startswith("NA_WN_")}
        r = subprocess.run([sys.executable, str(script)], env=dict(e, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        seen.add(r.stdout.strip())
    assert len(seen) == 1, seen
    assert seen.pop().split() == [str(na.snapshot_fingerprint(_load(na, "BossWN-nano.nam"))), str(FIXED_HEADER + SECTION_ENTRY + 4 * 8692)]


def test_save_without_a_device_fails_loudly(na):
    """There is no host-side stream state: without a HIP device a save reports an error, it never returns a blob of something."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = _load(na, "BossLSTM-1x16.nam")
    buf = C.create_string_buffer(4096)
    buf.raw = b"\x7f" * 4096
    written = C.c_size_t(77)
    ids = (C.c_int * 1)(0)
    # no batch can exist without a device (NA_BatchCreate fails): the entry point says so instead of crashing on the null handle
    assert lib.NA_BatchSaveStreams(None, ids, 1, buf, 4096, C.byref(written)) != 0
    assert "null batch" in capi.last_error() and written.value == 0
    assert lib.NA_BatchLoadStreams(None, ids, 1, buf, 4096) != 0
    assert "null batch" in capi.last_error()
    assert lib.NA_BatchStreamSnapshotBytes(None, 0) < 0
    assert lib.NA_SaveModelState(None, buf, 4096, C.byref(written)) != 0
    assert "model is null" in capi.last_error()
    if na.device_count() > 0:
        # with a device the same call works (the rest is tests/test_gpu_snapshot.py)
        assert lib.NA_SaveModelState(m._h, buf, 4096, C.byref(written)) == 0, capi.last_error()
        assert written.value == na.snapshot_bytes(m)
        return
    with pytest.raises(na.NeuralAudioError):
        na.Batch(0)
    assert lib.NA_SaveModelState(m._h, buf, 4096, C.byref(written)) != 0
    assert "no HIP device" in capi.last_error()
    assert written.value == 0 and buf.raw == b"\x7f" * 4096  # nothing was written
    assert lib.NA_LoadModelState(m._h, buf, 4096) != 0
    assert "no HIP device" in capi.last_error()
    with pytest.raises(na.NeuralAudioError):
        m.SaveState()
    # a second call fails the same way (no half-built device state left behind)
    assert lib.NA_SaveModelState(m._h, buf, 4096, C.byref(written)) != 0


def test_format_version_1_is_pinned_by_a_committed_blob(na):
    """tests/golden/snapshots/lstm_1x16_v1.bin: BossLSTM-1x16.nam after 1000 samples of O.signal_noise(1000, seed=7), written by
    NA_SaveModelState on an MI355X.  Layout, field order, sizes and the fingerprint of that file are version 1."""
    blob = open(GOLDEN_BLOB, "rb").read()
    m = _load(na, "BossLSTM-1x16.nam")
    head, sections = parse_snapshot(blob)
    assert head["magic"] == MAGIC and blob[:4] == b"NASS"
    assert head["version"] == 1
    assert head["total"] == len(blob) == FIXED_HEADER + SECTION_ENTRY + 4 * 32 == na.snapshot_bytes(m)
    assert head["fingerprint"] == na.snapshot_fingerprint(m)
    assert (head["nsub"], head["active"], head["flags"], head["prewarmed"]) == (1, 0, 0, 1)
    assert head["quality"] == 1.0
    assert head["header_bytes"] == FIXED_HEADER + SECTION_ENTRY
    (sec,) = sections
    assert (sec["kind"], sec["encoding"], sec["values"], sec["offset"]) == (KIND_LSTM, ENC_F32, 32, head["header_bytes"])
    state = sec["words"].view("<f4")
    # h then c of the one layer: |h| < 1 (o * tanh(c)), both finite and not the file's initial state any more
    assert np.all(np.isfinite(state)) and np.all(np.abs(state[:16]) < 1.0) and np.any(state != 0.0)
    w = np.asarray(O.load_json("BossLSTM-1x16.nam")["weights"], np.float32)
    H = 16
    h0 = w[4 * H * (1 + H) + 4 * H:4 * H * (1 + H) + 5 * H]
    assert not np.array_equal(state[:16], h0)
