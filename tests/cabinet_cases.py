"""Shared pieces of tests/test_gpu_cabinet.py: the cabinet stage's contract (include/neuralaudio_amd.h) restated in float64, the error
bounds, the hook batch and the scenario runner on the twelve-row batch of handover_cases.py.

Bounds.  u = 2^-24 is the unit roundoff of f32.  Any order of summing K f32 products in f32 (FMA or not) is within
(K + 4) * u * sum |h_k| |y_{t-k}| of the exact sum (the forward bound gamma_K, with four units to spare for the slices' joins): CONV_ABS
covers sums that are exactly zero.  A blended sample (1 - w) * c_A + w * c_B, with w and 1 - w computed in f32 as the contract does, adds
three roundings -- two products and a sum -- to the two convolution bounds weighted by (1 - w) and w."""
import copy
import ctypes as C

import numpy as np

import handover_cases as H

U = 2.0 ** -24
CONV_ABS = 1e-30
RAGGED = H.RAGGED


def conv64(h, y):
    """c_h[t] in float64 for a history that starts at y[0]"""
    return np.convolve(np.asarray(y, np.float64), np.asarray(h, np.float64))[:len(y)]


def conv_bound(h, y):
    K = len(h)
    return (K + 4) * U * conv64(np.abs(np.asarray(h, np.float64)), np.abs(np.asarray(y, np.float64))) + CONV_ABS


def sequential_f32(h, y):
    """the plain sequential f32 sum: acc = fl(acc + fl(h[k] * y[t - k])) for k = 0, 1, ..., for every t at once"""
    h, y = np.asarray(h, np.float32), np.asarray(y, np.float32)
    acc = np.zeros(len(y), np.float32)
    for k in range(len(h)):
        acc[k:] = acc[k:] + h[k] * y[:len(y) - k]
    return acc


def weight32(N, k):
    """w of the k-th sample of a fade of N, as the contract computes it in f32, and 1 - w"""
    k = np.asarray(k)
    w = np.where(k >= N - 1, np.float32(1.0), (np.minimum(k, N - 1) + 1).astype(np.float32) / np.float32(max(N, 1))).astype(np.float32)
    return w.astype(np.float64), (np.float32(1.0) - w).astype(np.float64)


class CabContract:
    """Which row has which IR, its history since T0 and its fade: the expected rows of a call in float64, their bounds, and which rows
    must be the input's bits."""

    def __init__(self, rows, irs):
        self.rows, self.irs = rows, irs  # irs: name -> taps (float32)
        self.state = {s: None for s in range(rows)}  # None: dry, no entry; else dict cur, frm, fading, N, k, hist

    def set_ir(self, s, ir, N):
        st = self.state[s]
        if st is None:
            if ir is None:
                return
            self.state[s] = dict(cur=ir, frm=None, fading=N > 0, N=N, k=0, hist=np.zeros(0))
            return
        assert not st["fading"]
        if N > 0:
            st.update(frm=st["cur"], cur=ir, fading=True, N=N, k=0)
        elif ir is None:
            self.state[s] = None
        else:
            st["cur"] = ir

    def leave(self, s):
        self.state[s] = None

    def remaining(self, s):
        st = self.state[s]
        return st["N"] - st["k"] if st and st["fading"] else 0

    def _side(self, st, ir, n):
        if ir is None:
            return st["hist"][-n:].copy(), np.zeros(n)
        h = self.irs[ir]
        return conv64(h, st["hist"])[-n:], conv_bound(h, st["hist"])[-n:]

    def step(self, y):
        """y: the rows of this call without the stage.  Returns (expected f64, bound, exact)."""
        n = y.shape[1]
        e, bound, exact = y.astype(np.float64), np.zeros(y.shape), np.ones(self.rows, bool)
        for s, st in self.state.items():
            if st is None:
                continue
            st["hist"] = np.concatenate([st["hist"], y[s].astype(np.float64)])[-(8192 + n):]
            c, b = self._side(st, st["cur"], n)
            if st["fading"]:
                cf, bf = self._side(st, st["frm"], n)
                w, v = weight32(st["N"], st["k"] + np.arange(n))
                b = v * bf + w * b + 3 * U * (v * (np.abs(cf) + bf) + w * (np.abs(c) + b)) + CONV_ABS
                c = v * cf + w * c
                st["k"] = min(st["k"] + n, st["N"])
                if st["k"] >= st["N"]:
                    st["fading"], st["frm"] = False, None
            e[s], bound[s], exact[s] = c, b, False
            if not st["fading"] and st["cur"] is None:
                self.state[s] = None
        return e, bound, exact


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class HookBatch:
    """`rows` rows (BossWN-nano streams that never run) with the stage enabled: the hook runs the stage on host rows."""

    def __init__(self, na, nano, rows, max_taps):
        self.b = na.Batch(0)
        assert self.b.AddStreams(nano, rows, doPrewarm=False) == 0
        self.b.EnableCabinetStage(max_taps)
        self.rows = rows

    def run(self, x, calls=None, stride=lambda n: n):
        """the stage over x[rows, total], cut into `calls`; every call's block has rows stride(n) floats apart"""
        calls = [x.shape[1]] if calls is None else calls
        assert sum(calls) == x.shape[1]
        out, pos = [], 0
        for n in calls:
            block = np.full((self.rows, stride(n)), np.float32(7.0))
            block[:, :n] = x[:, pos:pos + n]
            self.b.DebugRunCabinetStage(block, n)
            assert np.all(block[:, n:] == np.float32(7.0)), "the stage wrote past the end of a row"
            out.append(block[:, :n].copy())
            pos += n
        return np.concatenate(out, axis=1)

    def close(self):
        self.b.close()


def integers(rng, shape, lim):
    return rng.integers(-lim, lim + 1, shape).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the twelve-row batch of handover_cases.py with the stage: ops of H plus ("ir", stream, name or None, fade) ----

def make_batch(na, models, irs, max_taps, out_stage=False, resample=None, hip_stream=None):
    b = H.make_batch(na, models, stage=out_stage, resample=resample, hip_stream=hip_stream)
    b.EnableCabinetStage(max_taps)
    ids = {name: b.LoadIR(taps) for name, taps in irs.items()}
    return b, ids


def run_scenario(na, models, x, calls, ops, irs, max_taps=256, path="process", resample=None, out_stage=False, hook=None):
    """The batch under test through `path` against its twin (no stage at all) and the composed contract: the cabinet stage on the
    twin's rows, then the output stage's contract on that.  Returns (rows, twin rows, largest error / limit)."""
    twin_ops = {i: [op for op in v if op[0] != "ir"] for i, v in ops.items()}
    yts = H.run_twin(na, models, x, calls, twin_ops, resample)
    b, ids = make_batch(na, models, irs, max_taps, out_stage=out_stage, resample=resample)
    runner, cab, outc = H.Runner(na, b, path), CabContract(H.ROWS, irs), H.Contract()
    got, pos, worst = [], 0, 0.0
    try:
        for i, n in enumerate(calls):
            for op in ops.get(i, ()):
                if op[0] == "ir":
                    b.SetStreamIR(op[1], -1 if op[2] is None else ids[op[2]], op[3])
                    cab.set_ir(op[1], op[2], op[3])
                    continue
                H.drive(b, op, out_stage or op[0] not in ("gain", "handover"))
                outc.apply(op)
                if op[0] == "park" or (op[0] == "handover" and op[3] == 0):
                    cab.leave(op[1])
            y = runner.call(x[:, pos:pos + n])
            for f in outc.finished:  # (parked by this call, in front of its launches)
                cab.leave(f)
            z, zb, zexact = cab.step(yts[i])
            errs = copy.deepcopy(outc)
            e, bound, exact = outc.step(z)
            eb, _, _ = errs.step(zb)  # (the output stage is linear with weights >= 0: the cabinet's bound goes through it as a signal)
            for s in range(H.ROWS):
                what = (path, "call", i, "row", s)
                if s in outc.parked:
                    assert not np.any(y[s]), what
                elif exact[s] and zexact[s]:
                    assert np.array_equal(y[s], yts[i][s]), what + ("differs from the twin",)
                else:
                    err = np.abs(y[s].astype(np.float64) - e[s])
                    # the output stage does nothing to the row: the convolution's bound alone; else the cabinet's bound as the output
                    # stage passes it on (its own roundings on top) plus the output stage's own tolerance
                    limit = zb[s] if exact[s] else eb[s] * (1 + 4 * H.REL) + H.REL * bound[s] + H.ABS
                    worst = max(worst, float(np.max(err / limit)))
                    assert np.all(err <= limit), what + (int(np.argmax(err - limit)), float(np.max(err)), float(np.max(err / limit)))
            got.append(y)
            pos += n
            if hook:
                hook(b, cab, outc, i)
    finally:
        runner.close()
        b.close()
    return np.concatenate(got, axis=1), np.concatenate(yts, axis=1), worst
