#!/usr/bin/env python3
"""Time the streaming resampler (NA_BatchSetResampling): tools/quick_time_resample.py <mode> [streams] -- 1024 x A1 Standard by default,
calls of 128 external samples at 44.1 -> 48 kHz, device buffers, the library's timing marks; one JSON line.
  plain      an un-resampled batch, 128 frames per call (also under NA_LIB_SUFFIX: the same figure from another build)
  resampled  q = 32 and q = 1 beside the SAME build un-resampled over the model-side lengths each of them cycles through,
             alternating, three repetitions each; K calls per repetition, K a multiple of the 147-call phase period"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import neuralaudio_amd as na

mode = sys.argv[1]
S = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
FE, FM, N, STRIDE = 44100, 48000, 128, 256
K = 147 * int(os.environ.get("PERIODS", "4"))
dev = torch.device("cuda", 0)
m = na.NeuralModelLoader().CreateFromFile(os.path.join(ROOT, "tests/golden/models/BossWN-standard.nam"), doPrewarm=False)
x = torch.clamp(0.25 * torch.randn(S, STRIDE), -1, 1).to(dev)
y = torch.empty_like(x)
torch.cuda.synchronize()


def batch(q=None):
    b = na.Batch(0)
    if q is not None:
        b.SetResampling(FE, FM, quantum=q, max_frames=N)
    b.AddStreams(m, S)
    return b


def run(b, lengths):
    """us per call over the K calls of `lengths`"""
    b.MarkTime(0)
    for n in lengths:
        b.ProcessDevice(x.data_ptr(), y.data_ptr(), n, STRIDE, STRIDE)
    b.MarkTime(1)
    b.WaitMarks()
    us = b.ElapsedMs() / len(lengths) * 1e3
    b.Synchronize()
    return us


out = {"mode": mode, "streams": S, "calls": K, "lib": os.environ.get("NA_LIB_SUFFIX", "")}
if mode == "plain":
    b = batch()
    run(b, [N] * K)
    out["us_per_call"] = [round(run(b, [N] * K), 2) for _ in range(3)]
else:
    frames = {q: [na.resample_model_frames(FE, FM, q, N * (i + 1)) - na.resample_model_frames(FE, FM, q, N * i) for i in range(K)] for q in (32, 1)}
    cfg = {"q32": (batch(32), [N] * K), "q1": (batch(1), [N] * K), "plain_lengths_q32": (batch(), frames[32]), "plain_lengths_q1": (batch(), frames[1])}
    for b, lengths in cfg.values():
        run(b, lengths)
    res = {k: [] for k in cfg}
    for _ in range(3):
        for k, (b, lengths) in cfg.items():
            res[k].append(round(run(b, lengths), 2))
    out["us_per_call"] = res
    out["model_frames"] = {str(q): sorted(set(f)) for q, f in frames.items()}
print(json.dumps(out))
