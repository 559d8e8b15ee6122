#!/usr/bin/env python3
"""Which kernels the recurrent models launch: tools/recurrent_kernel_census.py  (run under `rocprofv3 --kernel-trace -- python ...`).

Loads a fixed list of recurrent shapes that spans every branch of the kernel decision (lstm_dev.h RecurrentKernelFor: the LDS-free
layouts, the shaped one-wave instances, the runtime-shaped kernel on one wave / a workgroup / L2-streamed weights / the head in the
loop, dense and conv1d tails, a stack without a recurrent layer) and processes ONE 16-sample buffer of three streams of each, in that
order, without prewarm.  The ordered list of dispatched kernel names in the trace is the census: two builds of the library launch the
same kernels if their lists are equal.  Tuning knobs (NA_LSTM_NO_DPP=1 NA_GRU_NO_DPP=1, NA_LSTM_LANE_KERNEL=1 ...) move shapes between
kernels; the printed lines say what NA_BatchStreamKernelName answers for each shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import neuralaudio_amd as na
import na_oracle as O
import ref_np as R

LSTM = [(1, 3), (1, 5), (1, 8), (1, 12), (1, 16), (1, 17), (1, 24), (1, 32), (1, 33), (1, 40), (1, 64), (1, 65), (1, 129), (1, 257),
        (2, 8), (2, 12), (2, 13), (2, 16), (2, 20), (2, 24), (2, 32), (2, 40), (2, 64), (3, 16), (3, 24)]
GRU = [(1, 5), (1, 8), (1, 16), (1, 20), (1, 21), (1, 22), (1, 24), (1, 32), (1, 86), (1, 171), (2, 8), (2, 12), (2, 16), (2, 20), (2, 24), (3, 16)]
STACKS = [[("lstm", 8), ("dense", 4, "tanh"), ("dense", 1)], [("gru", 12), ("dense", 5, "relu"), ("dense", 1)], [("dense", 8, "tanh"), ("dense", 1)],
          [("lstm", 8), ("conv1d", 6, 5, 3), ("dense", 1)], [("gru", 160), ("dense", 8, "tanh"), ("dense", 1)]]

loader = na.NeuralModelLoader()
x = np.stack([O.signal_noise(16, 5 + s) for s in range(3)])
models = [("lstm %dx%d" % s, O.nam_json_lstm(s[0], s[1], O.synth_lstm_weights(s[0], s[1], seed=9)), ".nam") for s in LSTM]
models += [("gru %dx%d" % s, json.dumps(O.synth_keras_gru(s[0], s[1], seed=9)), ".json") for s in GRU]
models += [("stack " + "-".join("%s%d" % (l[0], l[1]) for l in s), json.dumps(R.synth_keras_stack(s, seed=9)), ".json") for s in STACKS]
for name, doc, ext in models:
    m = loader.CreateFromString(doc, ext, doPrewarm=False)
    b = na.Batch(0)
    b.AddStreams(m, 3, doPrewarm=False)
    try:
        y = b.Process(x)
        print("%-28s %-24s finite %s" % (name, b.StreamKernelName(0), bool(np.isfinite(y).all())), flush=True)
    except na.NeuralAudioError as e:  # (a knob that leaves the shape without a kernel: the launch is refused, the census goes on)
        print("%-28s no kernel: %s" % (name, e), flush=True)
    b.close()
