"""Writes tests/golden/snapshots/lstm_1x16_v1.bin: the committed blob that pins format version 1 of the stream snapshots
(csrc/stream_snapshot.h; read by tests/test_snapshot_cpu.py with its own pure-Python parser).  Needs a GPU.  Run it again only for a
NEW format version, under a new file name: the blob of an old version stays as the compatibility fixture."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import neuralaudio_amd as na  # noqa: E402
import na_oracle as O  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "snapshots", "lstm_1x16_v1.bin")
    m = na.NeuralModelLoader().CreateFromFile(os.path.join(O.MODELS_DIR, "BossLSTM-1x16.nam"))
    m.Process(O.signal_noise(1000, seed=7))
    blob = m.SaveState()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "wb") as f:
        f.write(blob)
    print("wrote %d bytes to %s" % (len(blob), out))


if __name__ == "__main__":
    main()
