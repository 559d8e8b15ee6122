"""Shared pieces of tests/test_mix_cpu.py and tests/test_gpu_mix.py: the mix stage's contract (include/neuralaudio_amd.h, csrc/mix_stage.h)
restated in numpy float32, the batch every model case uses and its twin without the stage.

The restatement (MixRef) is one group: the gain function with its f64 quotient, the skip-zero sum in member order, and Reached -- the
gains of the last sample produced, which a set call during a ramp starts from.  Every numpy operation on float32 arrays is one
separately rounded f32 operation, which is the contract; comparisons against it are np.array_equal.

The batch is the one of tests/handover_cases.py -- BossWN-nano x 4 packed (rows 0-3), BossWN-standard (rows 4-7), BossLSTM-2x8 (rows
8-11), all from NA_BatchReserveStreams; rows 0, 1, 4, 5, 8, 9 live, the others parked -- with the output stage enabled (hand-overs)
and, for the batch under test, the mix stage.  The twin is the same batch without the mix stage."""
import ctypes as C

import numpy as np

import handover_cases as H

F = np.float32
OUT, DRY = 0, 1
MAX_MEMBERS = 8
ROWS, LIVE = H.ROWS, H.LIVE
NOT_ENABLED = "mix stage not enabled (NA_BatchEnableMixStage)"
# the contract's lines, as they stand in the public header (and, but for the comment's leading " * ", in csrc/mix_stage.h)
CONTRACT = [
    "g1 for k >= R - 1",
    "fl(g0 + fl(fl(g1 - g0) * w))",
    "w = (float)((double)(k + 1) / (double)R)",
    "acc = fl(g_dj * y_j) for the first",
    "acc = fl(acc + fl(g_dj * y_j)) for each further one",
    "+0.0f",
]


def gain_at(g0, g1, R, k):
    """[len(k), D, M] float32: the gains of every cell at the positions k (int64) of a ramp (R) from g0 to g1"""
    k = np.asarray(k, np.int64)
    g0, g1 = np.asarray(g0, F), np.asarray(g1, F)
    with np.errstate(all="ignore"):
        w = ((k + 1).astype(np.float64) / np.float64(max(R, 1))).astype(F)  # the f64 quotient, rounded once
        d = g1 - g0                                                         # fl(g1 - g0)
        p = d[None, :, :] * w[:, None, None]                                # fl(. * w)
        g = g0[None, :, :] + p                                              # fl(g0 + .)
    assert g.dtype == F
    g[k >= R - 1] = g1
    return g


def mix_sum(g, y):
    """g [n, D, M] float32, y [M, n] float32 -> [D, n] float32: the skip-zero sum in member order"""
    n, D, M = g.shape
    out, some = np.zeros((D, n), F), np.zeros((D, n), bool)
    with np.errstate(all="ignore"):
        for j in range(M):
            gj = np.ascontiguousarray(g[:, :, j].T)
            p = gj * y[j][None, :]
            s = np.where(some, out + p, p)
            live = gj != 0
            out = np.where(live, s, out).astype(F)
            some |= live
    return out


class MixRef:
    """One group: members (streams, taps), D outputs, the ramp and its two matrices."""

    def __init__(self, streams, gains, D=None, taps=None, R=0):
        self.streams = [int(s) for s in streams]
        self.M = len(self.streams)
        self.taps = [OUT] * self.M if taps is None else [int(t) for t in taps]
        g = np.asarray(gains, F)
        self.D = int(D) if D is not None else (g.shape[0] if g.ndim == 2 else 1)
        g = g.reshape(self.D, self.M)
        self.g1 = g.copy()
        self.g0 = np.eye(self.D, self.M, dtype=F) if R > 0 else g.copy()  # a new group starts from the identity
        self.R, self.k = int(R), 0

    def reached(self):
        """the gains of the last sample produced (none yet: what the ramp starts from)"""
        return self.g0.copy() if self.k == 0 else gain_at(self.g0, self.g1, self.R, [self.k - 1])[0]

    def set(self, gains, R=0):
        g = np.asarray(gains, F).reshape(self.D, self.M)
        self.g0 = self.reached() if R > 0 else g.copy()
        self.g1, self.R, self.k = g.copy(), int(R), 0

    def remaining(self):
        return self.R - self.k

    def gains(self, n):
        return gain_at(self.g0, self.g1, self.R, self.k + np.arange(n, dtype=np.int64))

    def run(self, rows, x=None):
        """rows [R, n]: the rows as the output stage left them (x: the input rows of the same call); returns the rows behind the stage"""
        rows = np.asarray(rows, F)
        n = rows.shape[1]
        y = np.stack([(x if t == DRY else rows)[s] for s, t in zip(self.streams, self.taps)]).astype(F)
        mixed = mix_sum(self.gains(n), y)
        out = rows.copy()
        for d in range(self.D):
            out[self.streams[d]] = mixed[d]
        self.k = min(self.R, self.k + n)
        return out


def run_groups(refs, rows, x=None):
    """every group on the same call: groups share no stream, so their order does not matter"""
    out = np.asarray(rows, F)
    for ref in refs:
        out = ref.run(out, x)
    return out


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def same_bits(a, b):
    """equality of bit patterns: NaN payloads and the sign of zero included"""
    return np.array_equal(bits(a), bits(b))


def make_batch(na, models, mix, output=True):
    b = H.make_batch(na, models, stage=output)
    if mix:
        b.EnableMixStage()
    return b


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def debug_run(b, rows, n, stride, x=None):
    """NA_DebugRunMixStage on [R, n] rows held `stride` floats apart; returns the rows behind the stage, and checks the padding"""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    R = rows.shape[0]
    pad = F(-7.5)
    buf = np.full((R, stride), pad, F)
    buf[:, :n] = rows
    xin = None
    if x is not None:
        xin = np.full((R, stride), pad, F)
        xin[:, :n] = x
    rc = lib.NA_DebugRunMixStage(b._h, fp(xin) if xin is not None else None, fp(buf), stride, n)
    assert rc == 0, capi.last_error()
    assert np.all(buf[:, n:] == pad), "the stage wrote past the end of a row"
    return buf[:, :n].copy()


def lstm_batch(na, models, rows, mix=True):
    """`rows` live BossLSTM-2x8 streams: the cheapest batch to hold rows for the arithmetic cases"""
    b = na.Batch(0)
    assert b.AddStreams(models[H.LSTM], rows) == 0
    if mix:
        b.EnableMixStage()
    return b
