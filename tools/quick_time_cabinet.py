#!/usr/bin/env python3
"""Kernel time of the cabinet stage from the library's event marks: tools/quick_time_cabinet.py [streams=1024] [frames=128] [steps=600]
A1 Standard streams on device pointers.  The batch's stream is handed out first (NA_BatchGetHipStream), so that every configuration runs
its launches in order on that one stream -- what a batch with an entry does anyway -- and the difference to the first line is the
stage's own work: table upload, append launch, convolve launch.  Prints one JSON line per configuration: us per step between the
marks (NA_BatchMarkTime / NA_BatchElapsedMs), the stage's share, and the FMA rate of that share against the FP32 vector peak of the
MI355X (256 CUs x 128 FMA lanes x 2.4 GHz = 78.6 TFMA/s)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import neuralaudio_amd as na

S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
n = int(sys.argv[2]) if len(sys.argv) > 2 else 128
K = int(sys.argv[3]) if len(sys.argv) > 3 else 600
PEAK_FMA = 256 * 128 * 2.4e9
dev = torch.device("cuda", 0)
loader = na.NeuralModelLoader()
model = loader.CreateFromFile(os.path.join(ROOT, "tests", "golden", "models", "BossWN-standard.nam"), doPrewarm=False)
rng = np.random.default_rng(1)
x = torch.from_numpy(np.clip(0.25 * rng.standard_normal((4, S, n)), -1, 1).astype(np.float32)).to(dev)
y = torch.empty(S, n, device=dev)


def ir(taps, seed):
    r = np.random.default_rng(seed)
    return (0.1 * r.standard_normal(taps) * np.exp(-6.0 * np.arange(taps) / taps)).astype(np.float32)


def timed(b):
    for i in range(100):
        b.ProcessDevice(x[i % 4].data_ptr(), y.data_ptr(), n, n, n)
    b.Synchronize()
    b.MarkTime(0); b.MarkTime(1)
    torch.cuda.synchronize(dev)
    b.MarkTime(0)
    for i in range(K):
        b.ProcessDevice(x[i % 4].data_ptr(), y.data_ptr(), n, n, n)
    b.MarkTime(1); b.WaitMarks()
    torch.cuda.synchronize(dev)
    us = b.ElapsedMs() * 1e3 / K
    b.Synchronize()
    return us


def batch(max_taps):
    b = na.Batch(0)
    b.AddStreams(model, S)
    b.GetHipStream()  # ordered launches on the batch stream from here on
    if max_taps:
        b.EnableCabinetStage(max_taps)
    return b


def report(name, us, base, macs):
    stage = us - base
    line = {"config": name, "streams": S, "frames": n, "steps": K, "us_per_step": round(us, 2), "stage_us": round(stage, 2)}
    if macs:
        line.update(gmac_per_step=round(macs * 1e-9, 4), tfma_per_s=round(macs / (stage * 1e-6) * 1e-12, 2), of_fp32_vector_peak=round(macs / (stage * 1e-6) / PEAK_FMA, 4))
    print(json.dumps(line), flush=True)


b = batch(0)
base = timed(b)
report("ordered launches, no stage", base, base, 0)
b.close()
b = batch(4096)
report("stage enabled, no IR", timed(b), base, 0)
shared = b.LoadIR(ir(2048, 5))
for s in range(S):
    b.SetStreamIR(s, shared, 0)
report("one shared 2048-tap IR on every stream", timed(b), base, S * n * 2048)
for s in range(S):
    b.SetStreamIR(s, -1, 0)
b.UnloadIR(shared)
ids = [b.LoadIR(ir(4096, 100 + s)) for s in range(S)]
for s in range(S):
    b.SetStreamIR(s, ids[s], 0)
report("%d distinct 4096-tap IRs" % S, timed(b), base, S * n * 4096)
for s in range(S):
    b.SetStreamIR(s, ids[s] if s < 16 else -1, 0)
b.ProcessDevice(x[0].data_ptr(), y.data_ptr(), n, n, n)
for s in range(16):
    b.SetStreamIR(s, ids[s + 16], 1 << 20)
report("sixteen concurrent fades between 4096-tap IRs", timed(b), base, 16 * n * 4096 * 2)
b.close()
