"""Shared pieces of tests/test_reverb_cpu.py and tests/test_gpu_reverb.py: the reverb stage's contract (include/neuralaudio_amd.h,
csrc/reverb_stage.h) restated in numpy float32, operation for operation, and the hook batch.

Every numpy expression below is one f32 ufunc call on f32 arrays: one rounding to nearest even per operation, no FMA, subnormals kept --
what the contract states for the device.  The twiddle table is an argument: the GPU tests pass the library's own (NA_DebugReverbTwiddles),
the CPU tests the one numpy computes (twiddles_numpy), which agrees with it to within one f32 ulp.

reverb_f32(h, x, tw, wet, dry) is the whole output of one setting on a history that starts at T0 = x[0].  The spectra X_m do not depend
on the IR, so the output of a setting after a switch is this function on the whole history since T0, from the switch on: class
RevContract keeps the histories and the fades and blends as the contract does."""
import ctypes as C

import numpy as np

P = 128
POINTS = 2 * P
PIECE = 1024
MAX_TAPS = 131072
F = np.float32
BITREV = np.array([int(format(i, "08b")[::-1], 2) for i in range(POINTS)])


def twiddles_numpy():
    """W[q] = (cos(2 pi q / 256), -sin(2 pi q / 256)) in double, rounded to f32: [2q], [2q + 1]"""
    a = 2.0 * np.pi * np.arange(P) / POINTS
    return np.stack([np.cos(a), -np.sin(a)], axis=1).astype(F).reshape(-1)


def cmul(ar, ai, br, bi):
    """four multiplies, one subtract, one add"""
    ac, bd, ad, bc = ar * br, ai * bi, ar * bi, ai * br
    return ac - bd, ad + bc


def transform(re, im, tw, inverse=False):
    """F (or F', unscaled) over the last axis of f32 arrays [..., 256]: bit reversal, then eight stages of 128 butterflies"""
    assert re.dtype == F and im.dtype == F and tw.dtype == F and re.shape[-1] == POINTS
    re, im = re[..., BITREV].copy(), im[..., BITREV].copy()
    wr_all, wi_all = tw[0::2], (-tw[1::2] if inverse else tw[1::2])
    i = np.arange(P)
    for s in range(1, 9):
        half = 1 << (s - 1)
        j = i & (half - 1)
        top = ((i - j) << 1) + j
        bot = top + half
        q = j << (8 - s)
        pr, pi = cmul(wr_all[q], wi_all[q], re[..., bot], im[..., bot])
        ar, ai = re[..., top], im[..., top]
        re[..., bot], im[..., bot] = ar - pr, ai - pi
        re[..., top], im[..., top] = ar + pr, ai + pi
    return re, im


def ir_spectra(h, tw):
    """H_1 .. H_{J-1} of the taps h: (re, im) of shape [J - 1, 256]"""
    h = np.asarray(h, F)
    J = (len(h) + P - 1) // P
    padded = np.zeros(J * P, F)
    padded[:len(h)] = h
    win = np.zeros((max(J - 1, 0), POINTS), F)
    win[:, :P] = padded.reshape(J, P)[1:]
    return transform(win, np.zeros_like(win), tw)


def input_spectra(x, tw):
    """X_m of every complete block m of x (x[0] is T0): (re, im) of shape [blocks, 256]"""
    x = np.asarray(x, F)
    blocks = len(x) // P
    padded = np.concatenate([np.zeros(P, F), x[:blocks * P]])
    win = np.stack([padded[m * P:m * P + POINTS] for m in range(blocks)]) if blocks else np.zeros((0, POINTS), F)
    return transform(win, np.zeros_like(win), tw)


def head_f32(h, x, start=0):
    """sum over k < min(K, 128), k <= t, rising k from +0, a multiply and then an add: for t >= start"""
    h, x = np.asarray(h, F), np.asarray(x, F)
    acc = np.zeros(len(x), F)
    for k in range(min(len(h), P)):
        lo = max(k, start)
        if lo < len(x):
            acc[lo:] = acc[lo:] + h[k] * x[lo - k:len(x) - k]
    return acc[start:]


def tails_f32(h, x, tw, first_block=0):
    """the tails of blocks first_block .. (len(x) - 1) // 128 as one array, block after block"""
    x = np.asarray(x, F)
    Hr, Hi = ir_spectra(h, tw)
    Xr, Xi = input_spectra(x, tw)
    blocks = (len(x) + P - 1) // P
    need = np.arange(first_block, blocks)
    ar, ai = np.zeros((len(need), POINTS), F), np.zeros((len(need), POINTS), F)
    for j in range(1, Hr.shape[0] + 1):  # rising j; block b takes the term when j <= b
        sel = need >= j
        if not np.any(sel):
            break
        pr, pi = cmul(Hr[j - 1], Hi[j - 1], Xr[need[sel] - j], Xi[need[sel] - j])
        ar[sel], ai[sel] = ar[sel] + pr, ai[sel] + pi
    re, _ = transform(ar, ai, tw, inverse=True)
    return (re[:, P:] * F(2.0 ** -8)).reshape(-1)


def reverb_f32(h, x, tw, wet=1.0, dry=0.0, start=0):
    """y[start:] of the setting (h, wet, dry) on the history x since T0 (the defaults: the convolution alone)"""
    x = np.asarray(x, F)
    b0 = start // P
    tail = tails_f32(h, x, tw, b0)[start - b0 * P:][:len(x) - start]
    c = head_f32(h, x, start) + tail
    return F(dry) * x[start:] + F(wet) * c


def weight32(N, k):
    """OutStageWeightAt in f32"""
    k = np.asarray(k)
    return np.where(k >= N - 1, F(1.0), (np.minimum(k, max(N - 1, 0)) + 1).astype(F) / F(max(N, 1))).astype(F)


def blend_f32(w, a, b):
    """y_B where w = 1, else ((1 - w) * y_A) + (w * y_B)"""
    return np.where(w == F(1.0), b, (F(1.0) - w) * a + w * b).astype(F)


def expected_launches(t, calls, have=False):
    """launches of the calls for entries that all stand at position t: per piece the append and apply launches, the spectrum launch
    where the piece completes a block, the tail launch where it touches a block whose tail does not exist yet"""
    total = 0
    for n in calls:
        done = 0
        while done < n:
            piece = min(PIECE, n - done)
            o = (t + done) % P
            touched = (o + piece - 1) // P + 1
            exists = o != 0 and (done > 0 or have)
            total += 2 + (1 if (o + piece) // P > 0 else 0) + (1 if touched - (1 if exists else 0) > 0 else 0)
            done += piece
        t, have = t + n, True
    return total


class RevContract:
    """Which row has which setting (IR name, wet, dry), its history since T0 and its fade: the expected f32 rows of a call and which
    rows must be the input's bits."""

    def __init__(self, rows, irs, tw):
        self.rows, self.irs, self.tw = rows, irs, tw  # irs: name -> taps (float32)
        self.state = {s: None for s in range(rows)}   # None: no entry; else dict cur, frm (None or (ir, wet, dry)), fading, N, k, hist

    def set(self, s, ir, wet=1.0, dry=0.0, N=0):
        new = None if ir is None else (ir, wet, dry)
        st = self.state[s]
        if st is None:
            if new is None:
                return
            self.state[s] = dict(cur=new, frm=None, fading=N > 0, N=N, k=0, hist=np.zeros(0, F))
            return
        assert not st["fading"]
        if N > 0:
            st.update(frm=st["cur"], cur=new, fading=True, N=N, k=0)
        elif new is None:
            self.state[s] = None
        else:
            st["cur"] = new

    def leave(self, s):
        self.state[s] = None

    def remaining(self, s):
        st = self.state[s]
        return st["N"] - st["k"] if st and st["fading"] else 0

    def _side(self, st, setting, n):
        hist = st["hist"]
        if setting is None:
            return hist[len(hist) - n:].copy()
        ir, wet, dry = setting
        return reverb_f32(self.irs[ir], hist, self.tw, wet, dry, start=len(hist) - n)

    def step(self, x):
        """x: the rows of this call in front of the stage.  Returns (expected f32, exact)."""
        n = x.shape[1]
        e, exact = x.astype(F).copy(), np.ones(self.rows, bool)
        for s, st in self.state.items():
            if st is None:
                continue
            st["hist"] = np.concatenate([st["hist"], x[s].astype(F)])
            y = self._side(st, st["cur"], n)
            if st["fading"]:
                y = blend_f32(weight32(st["N"], st["k"] + np.arange(n)), self._side(st, st["frm"], n), y)
                st["k"] = min(st["k"] + n, st["N"])
                if st["k"] >= st["N"]:
                    st["fading"], st["frm"] = False, None
            e[s], exact[s] = y, False
            if not st["fading"] and st["cur"] is None:
                self.state[s] = None
        return e, exact


def library_twiddles():
    from neuralaudio_amd import capi
    tw = np.zeros(POINTS, F)
    assert capi.load_library().NA_DebugReverbTwiddles(tw.ctypes.data_as(C.POINTER(C.c_float)), POINTS) == POINTS
    return tw


class HookBatch:
    """`rows` rows (BossWN-nano streams that never run) with the stage enabled: the hook runs the stage on host rows."""

    def __init__(self, na, nano, rows, max_taps):
        self.b = na.Batch(0)
        assert self.b.AddStreams(nano, rows, doPrewarm=False) == 0
        self.b.EnableReverbStage(max_taps)
        self.rows = rows

    def run(self, x, calls=None, stride=lambda n: n):
        """the stage over x[rows, total], cut into `calls`; every call's block has rows stride(n) floats apart"""
        calls = [x.shape[1]] if calls is None else calls
        assert sum(calls) == x.shape[1]
        out, pos = [], 0
        for n in calls:
            block = np.full((self.rows, stride(n)), F(7.0))
            block[:, :n] = x[:, pos:pos + n]
            self.b.DebugRunReverbStage(block, n)
            assert np.all(block[:, n:] == F(7.0)), "the stage wrote past the end of a row"
            out.append(block[:, :n].copy())
            pos += n
        return np.concatenate(out, axis=1)

    def close(self):
        self.b.close()


def integers(rng, shape, lim):
    return rng.integers(-lim, lim + 1, shape).astype(F)


def decaying(rng, K):
    """normal taps under an exp(-k / (K/4)) decay"""
    return (rng.standard_normal(K) * np.exp(-np.arange(K) / (K / 4.0))).astype(F)


def conv64(h, x):
    return np.convolve(np.asarray(x, np.float64), np.asarray(h, np.float64))[:len(x)]


def rel_rms(y, ref):
    return float(np.sqrt(np.mean((np.asarray(y, np.float64) - ref) ** 2) / np.mean(ref ** 2)))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))
