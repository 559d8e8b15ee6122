"""The lines of profiles/wide_gated_cost.txt: us per step of 256 streams x 128 frames of an A1-shaped model of C / C/2 channels, event marks
around 200 ProcessDevice calls, five runs.  python tools/wide_gated_cost.py default|exact|gated C  (NA_LIB_SUFFIX=_x: tools/variants/ library)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import gated_cases as GC
import na_oracle as O
import neuralaudio_amd as na

mode, C = sys.argv[1], int(sys.argv[2])
STREAMS, N, WARM, CALLS, RUNS = 256, 128, 50, 200, 5
arrays = O.a1_arrays(C, C // 2, lite=False)
ld = na.NeuralModelLoader()
if mode == "gated":
    for a in arrays:
        a["gated"] = True
    ld.SetWaveNetWideGated(True)
    text = GC.nam_json(arrays, GC.weights(dict(arrays=arrays, seed=7)))
else:
    if mode == "exact":
        ld.SetWaveNetExactF32(True)
    text = O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=7))
m = ld.CreateFromString(text, ".nam")
b = na.Batch(0)
b.AddStreams(m, STREAMS)
x = torch.from_numpy(np.stack([O.signal_noise(N, 100 + s) for s in range(STREAMS)])).cuda()
y = torch.empty_like(x)
torch.cuda.synchronize()
times = []
for run in range(RUNS + 1):
    calls = WARM if run == 0 else CALLS
    b.MarkTime(0)
    for _ in range(calls):
        b.ProcessDevice(x.data_ptr(), y.data_ptr(), N)
    b.MarkTime(1)
    b.WaitMarks()
    if run:
        times.append(1000.0 * b.ElapsedMs() / calls)
assert bool(torch.isfinite(y).all())
print("%-8s %-8s %3d / %-3d %-22s %s" % (os.environ.get("NA_LIB_SUFFIX", "this") or "this", mode, C, C // 2, b.StreamKernelName(0), "  ".join("%6.1f" % t for t in times)), flush=True)
b.close()
