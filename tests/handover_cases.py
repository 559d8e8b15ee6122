"""Shared pieces of tests/test_gpu_handover.py: the batch every case uses, its twin, and the output stage's contract restated in float64.

The batch: three model families, one of them packed -- BossWN-nano (rows 0-3, four to a virtual stream), BossWN-standard (rows 4-7) and
BossLSTM-2x8 (rows 8-11), all from NA_BatchReserveStreams; rows 0, 1, 4, 5, 8, 9 are live, the others parked.  The TWIN has the same
reserve / activate / park history, no output stage, and keeps both streams of a hand-over running: its rows are y_from and y_to.  The
expected row is the formula of include/neuralaudio_amd.h evaluated in float64 on the twin's rows (class Contract).

A scenario is a list of call lengths and, per call index, the operations issued in front of that call:
  ("gain", stream, gain, ramp)  ("handover", from, to, fade)  ("park", stream)  ("activate", stream)"""
import ctypes as C
import os

import numpy as np

import na_oracle as O

NANO, STD, LSTM = "BossWN-nano.nam", "BossWN-standard.nam", "BossLSTM-2x8.nam"
ROWS = 12
FIRST = {NANO: 0, STD: 4, LSTM: 8}
LIVE = (0, 1, 4, 5, 8, 9)
RAGGED = [1, 15, 17, 64, 128, 129, 300]
REL, ABS = 1e-6, 1e-9  # |y - e| <= 1e-6 * (|g_from * y_from| + |g_to * y_to|) + 1e-9: six f32 roundings per term at the most, ~16 ulp


def noise(n, seed, gain=0.25):
    rng = np.random.default_rng(seed)
    return np.clip(gain * rng.standard_normal(n), -1.0, 1.0).astype(np.float32)


def load_models(na):
    loader = na.NeuralModelLoader()
    models = {name: loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False) for name in (NANO, STD, LSTM)}
    assert all(m is not None for m in models.values())
    models["loader"] = loader
    return models


def model_of(row):
    return NANO if row < 4 else (STD if row < 8 else LSTM)


def make_batch(na, models, stage, resample=None, hip_stream=None):
    b = na.Batch(0, hip_stream=hip_stream) if hip_stream is not None else na.Batch(0)
    if resample:
        b.SetResampling(resample)
    for name in (NANO, STD, LSTM):
        assert b.ReserveStreams(models[name], 4) == FIRST[name]
    assert b.StreamPackFactor(0) == 4, "the nano fixture runs four to a virtual stream"
    for s in LIVE:
        b.ActivateStream(s, 1.0)
    if stage:
        b.EnableOutputStage()
    return b


def signal(total, seed=0, same=()):
    """[ROWS, total] clipped noise; `same`: (from, to) pairs that are fed the same input (the host contract of a hand-over)"""
    x = np.stack([noise(total, 1000 * seed + 17 * r + 3) for r in range(ROWS)])
    for f, t in same:
        x[t] = x[f]
    return x


def ragged(total):
    """call lengths from RAGGED, in turn, that add up to `total`"""
    calls, left, i = [], total, 0
    while left > 0:
        n = min(RAGGED[i % len(RAGGED)], left)
        calls.append(n)
        left -= n
        i += 1
    return calls


class Contract:
    """The arithmetic of the header in float64, and who is parked: what every row of the batch must carry, call by call."""

    def __init__(self, rows=ROWS, live=LIVE):
        self.rows = rows
        self.ramp = {s: dict(a=1.0, b=1.0, R=0, k=0) for s in range(rows)}
        self.fades = []  # dicts f, t, N, k
        self.finished = []
        self.parked = set(range(rows)) - set(live)

    def _gain(self, s, k):
        r = self.ramp[s]
        k = np.asarray(k, np.float64)
        if r["R"] == 0:
            return np.full(k.shape, r["b"])
        return r["a"] + (r["b"] - r["a"]) * ((np.minimum(k, r["R"] - 1) + 1) / r["R"])

    def reached(self, s):
        r = self.ramp[s]
        return r["a"] if r["k"] == 0 else float(self._gain(s, r["k"] - 1))

    def in_fade(self, s):
        return any(s in (fd["f"], fd["t"]) for fd in self.fades)

    def remaining(self, s):
        return next((fd["N"] - fd["k"] for fd in self.fades if s in (fd["f"], fd["t"])), 0)

    def apply(self, op):
        if op[0] == "gain":
            _, s, g, R = op
            g = float(np.float32(g))
            self.ramp[s] = dict(a=self.reached(s) if R > 0 else g, b=g, R=R, k=0)
        elif op[0] == "handover":
            _, f, t, N = op
            self.parked.discard(t)
            if N == 0:
                self.apply(("park", f))
            else:
                self.fades.append(dict(f=f, t=t, N=N, k=0))
        elif op[0] == "park":
            s = op[1]
            self.fades = [fd for fd in self.fades if s not in (fd["f"], fd["t"])]
            self.finished = [f for f in self.finished if f != s]
            self.ramp[s] = dict(a=1.0, b=1.0, R=0, k=0)
            self.parked.add(s)
        elif op[0] == "activate":
            self.parked.discard(op[1])
        else:
            raise KeyError(op)

    def step(self, y):
        """y: the twin's rows of this call.  Returns (expected f64, bound, exact): exact rows must be the twin's bits (or zeros where
        parked), the others lie within REL * bound + ABS."""
        for f in self.finished:
            self.apply(("park", f))
        self.finished = []
        n = y.shape[1]
        y64 = y.astype(np.float64)
        e, bound, exact = y64.copy(), np.abs(y64), np.ones(self.rows, bool)
        idx = np.arange(n)
        scaled = {}
        for s in range(self.rows):
            r = self.ramp[s]
            scaled[s] = self._gain(s, r["k"] + idx) * y64[s]
            if r["b"] != 1.0 or r["k"] < r["R"]:
                e[s], bound[s], exact[s] = scaled[s], np.abs(scaled[s]), False
        for fd in self.fades:
            w = (np.minimum(fd["k"] + idx, fd["N"] - 1) + 1) / fd["N"]
            a, b = scaled[fd["f"]], scaled[fd["t"]]
            e[fd["t"]] = (1.0 - w) * a + w * b
            bound[fd["t"]] = np.abs(a) + np.abs(b)
            exact[fd["t"]] = False
        for s in self.parked:
            e[s], bound[s], exact[s] = 0.0, 0.0, True
        for r in self.ramp.values():
            r["k"] = min(r["k"] + n, r["R"])
            if r["k"] >= r["R"]:
                r["a"] = r["b"]
        for fd in self.fades:
            fd["k"] += n
        self.finished += [fd["f"] for fd in self.fades if fd["k"] >= fd["N"]]
        self.fades = [fd for fd in self.fades if fd["k"] < fd["N"]]
        return e, bound, exact


def drive(batch, op, stage):
    """one operation on the batch under test (stage) or on its twin (no stage: gains do nothing, a hand-over is the activation alone)"""
    if op[0] == "gain":
        if stage:
            batch.SetStreamGain(op[1], op[2], op[3])
    elif op[0] == "handover":
        if stage:
            batch.Handover(op[1], op[2], 1.0, op[3])
        else:
            batch.ActivateStream(op[2], 1.0)
    elif op[0] == "park":
        if stage or not batch.IsParked(op[1]):
            batch.ParkStream(op[1])
    elif op[0] == "activate":
        if stage or batch.IsParked(op[1]):
            batch.ActivateStream(op[1], 1.0)
    else:
        raise KeyError(op)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Runner:
    """Feeds a batch call by call through one entry point; every call returns host rows [ROWS, n] (device paths: copied back)."""

    def __init__(self, na, batch, path):
        self.na, self.b, self.path = na, batch, path
        self.reg = None
        if path in ("device", "device-odd"):
            import torch
            self.torch, self.dev = torch, torch.device("cuda", 0)

    def call(self, x):
        from neuralaudio_amd import capi
        lib, b = capi.load_library(), self.b
        x = np.ascontiguousarray(x)
        rows, n = x.shape
        if self.path == "process":
            return b.Process(x)
        if self.path == "submit":
            return b.Collect(b.Submit(x))
        if self.path == "registered":
            if self.reg is None or self.reg.shape[2] != n:
                self.close()
                self.reg = np.zeros((2, rows, n), np.float32)
                assert lib.NA_RegisterHostBuffer(self.reg.ctypes.data_as(C.c_void_p), self.reg.nbytes) == 0
            self.reg[0] = x
            assert lib.NA_BatchProcess(b._h, _fp(self.reg[0]), _fp(self.reg[1]), n) == 0, capi.last_error()
            return self.reg[1].copy()
        # device pointers: an output stride of n + 3 (rows that are not 16-byte aligned: the stage's scalar path) or of n rounded up to 4
        torch = self.torch
        stride = n + 3 if self.path == "device-odd" else (n + 3) // 4 * 4
        dx = torch.from_numpy(x).to(self.dev)
        dy = torch.zeros(rows, stride, device=self.dev)
        torch.cuda.synchronize(self.dev)
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, stride)
        b.Synchronize()
        out = dy.cpu().numpy()
        assert not np.any(out[:, n:]), "the stage wrote past the end of a row"
        return out[:, :n].copy()

    def close(self):
        if self.reg is not None:
            from neuralaudio_amd import capi
            assert capi.load_library().NA_UnregisterHostBuffer(self.reg.ctypes.data_as(C.c_void_p)) == 0
            self.reg = None


def run_twin(na, models, x, calls, ops, resample=None):
    """the twin's rows, call by call"""
    twin = make_batch(na, models, stage=False, resample=resample)
    out, pos = [], 0
    for i, n in enumerate(calls):
        for op in ops.get(i, ()):
            drive(twin, op, False)
        out.append(twin.Process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    twin.close()
    return out


def check_call(y, yt, contract, what, device_rows=False):
    """one call's rows against the contract; returns the largest error in units of the bound (printed by the callers)"""
    e, bound, exact = contract.step(yt)
    worst = 0.0
    for s in range(y.shape[0]):
        if s in contract.parked:
            # (host paths: silence; device rows of a parked stream are left alone -- the runner's zero-filled tensor)
            assert not np.any(y[s]), (what, "parked row", s)
        elif exact[s]:
            assert np.array_equal(y[s], yt[s]), (what, "row", s, "differs from the twin", int(np.count_nonzero(y[s] != yt[s])))
        else:
            err = np.abs(y[s].astype(np.float64) - e[s])
            limit = REL * bound[s] + ABS
            worst = max(worst, float(np.max(err / limit)))
            assert np.all(err <= limit), (what, "row", s, "sample", int(np.argmax(err - limit)), float(np.max(err)), float(np.max(err / limit)))
    return worst


def run_scenario(na, models, x, calls, ops, path="process", resample=None, hook=None, hip_stream=None):
    """The batch under test through `path` against its twin and the contract.  hook(batch, contract, i) runs after call i.  Returns
    (rows [ROWS, total], the twin's rows, the largest error / limit)."""
    yts = run_twin(na, models, x, calls, ops, resample)
    b = make_batch(na, models, stage=True, resample=resample, hip_stream=hip_stream)
    runner, contract = Runner(na, b, path), Contract()
    got, pos, worst = [], 0, 0.0
    try:
        for i, n in enumerate(calls):
            for op in ops.get(i, ()):
                drive(b, op, True)
                contract.apply(op)
            y = runner.call(x[:, pos:pos + n])
            worst = max(worst, check_call(y, yts[i], contract, (path, "call", i, "n", n)))
            got.append(y)
            pos += n
            if hook:
                hook(b, contract, i)
    finally:
        runner.close()
        b.close()
    return np.concatenate(got, axis=1), np.concatenate(yts, axis=1), worst
