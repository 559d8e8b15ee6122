#!/usr/bin/env python3
"""Time offline rendering at an external rate: tools/quick_time_offline_resample.py <at_rate|plain> [seconds] -- A1 Standard, host to
host, pageable buffers; one JSON line.
  at_rate  `seconds` of signal at 44.1 kHz through NA_RenderOfflineAtRate
  plain    the same M = J(N + L) model-rate samples through NA_RenderOffline (also under NA_LIB_SUFFIX: another build's figure)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import neuralaudio_amd as na

mode = sys.argv[1]
seconds = int(sys.argv[2]) if len(sys.argv) > 2 else 60
FE, FM = 44100, 48000
REPS = int(os.environ.get("REPS", "7"))
m = na.NeuralModelLoader().CreateFromFile(os.path.join(ROOT, "tests/golden/models/BossWN-standard.nam"), doPrewarm=False)
N = FE * seconds
L = na.resample_plan(FE, FM, 1)["latency_samples"]
M = na.resample_model_frames(FE, FM, 1, N + L)
n = N if mode == "at_rate" else M
x = np.sin(np.arange(n, dtype=np.float64) * 0.01).astype(np.float32)
kw = {"external_rate": FE} if mode == "at_rate" else {}
na.render_offline(m, x[:FE], **kw)
na.render_offline(m, x, **kw)
ms = []
for _ in range(REPS):
    t0 = time.perf_counter()
    na.render_offline(m, x, **kw)
    ms.append(round(1e3 * (time.perf_counter() - t0), 2))
print(json.dumps({"mode": mode, "seconds": seconds, "samples": n, "model_frames": M, "lib": os.environ.get("NA_LIB_SUFFIX", ""), "ms": ms,
                  "median_ms": float(np.median(ms))}))
