"""The modulation stage's contract (include/neuralaudio_amd.h, csrc/mod_stage.h) restated in numpy float32 and integers, operation for
operation, and the cases tests/test_mod_cpu.py (the header's step functions and book, no device) and tests/test_gpu_mod.py (the C ABI
on the device) share.  Every floating-point operation below is one numpy float32 operation, so each is rounded separately; nothing is
contracted; subnormals are kept.

The restatement does not use the chunk rule of the kernel: where no setting of a fade feeds back, w = x' is known up front and a call
is evaluated as arrays; as soon as one does, it walks the call sample by sample."""
import math

import numpy as np

F = np.float32
TRIANGLE, SINE = 0, 1
PIECE = 2048          # pieceSamples
MAX_DELAY = 4096      # the largest maxDelaySamples
PAD = MAX_DELAY + 8   # zeros in front of the line: w[t] = +0 for t < 0
FIELDS = ("baseSamples", "depthSamples", "phaseInc", "shape", "numVoices", "voicePhase", "voiceGain", "feedback", "wet", "dry", "tremoloDepth")


def params(base, depth=0.0, phase_inc=0, shape=TRIANGLE, voices=1, voice_phase=(0, 0, 0, 0), voice_gain=None, feedback=0.0, wet=1.0, dry=1.0, tremolo=0.0):
    """a dict of the NA_ModParams fields; floats already float32"""
    if voice_gain is None:
        voice_gain = [1.0 / voices if v < voices else 0.0 for v in range(4)]
    return dict(baseSamples=float(F(base)), depthSamples=float(F(depth)), phaseInc=int(phase_inc) & 0xFFFFFFFF, shape=int(shape), numVoices=int(voices),
                voicePhase=[int(v) & 0xFFFFFFFF for v in voice_phase], voiceGain=[float(F(g)) for g in voice_gain], feedback=float(F(feedback)),
                wet=float(F(wet)), dry=float(F(dry)), tremoloDepth=float(F(tremolo)))


def phase_inc(rate_hz, sample_rate=48000):
    return int(math.floor(rate_hz / sample_rate * 4294967296.0 + 0.5))


def from_ms(sample_rate, base_ms, depth_ms, rate_hz, shape, voices, feedback, wet_db, dry_db, tremolo):
    """NA_ModParamsFromMs in Python floats (double), each value rounded once"""
    gain = lambda db: 0.0 if db == float("-inf") else float(F(math.pow(10.0, db / 20.0)))
    return dict(baseSamples=float(F(base_ms * sample_rate / 1000.0)), depthSamples=float(F(depth_ms * sample_rate / 1000.0)),
                phaseInc=phase_inc(rate_hz, sample_rate), shape=shape, numVoices=voices,
                voicePhase=[int(math.floor(v * 4294967296.0 / voices)) if v < voices else 0 for v in range(4)],
                voiceGain=[float(F(1.0 / voices)) if v < voices else 0.0 for v in range(4)], feedback=float(F(feedback)), wet=gain(wet_db), dry=gain(dry_db),
                tremoloDepth=float(F(tremolo)))


def error(p, max_delay=MAX_DELAY):
    """None: fine; else the text of the first rule the constants break (ModParamsError)"""
    fin = lambda v: math.isfinite(v)
    if not fin(p["baseSamples"]) or p["baseSamples"] < 2.0:
        return "baseSamples must be finite and at least 2"
    if not fin(p["depthSamples"]) or p["depthSamples"] < 0.0:
        return "depthSamples must be finite and at least 0"
    if not (F(p["baseSamples"]) + F(p["depthSamples"]) <= F(max_delay - 2)):
        return "baseSamples + depthSamples must be at most maxDelaySamples - 2"
    if p["shape"] not in (TRIANGLE, SINE):
        return "shape must be NA_MOD_TRIANGLE or NA_MOD_SINE"
    if not 1 <= p["numVoices"] <= 4:
        return "numVoices must lie in [1, 4]"
    for v in range(4):
        if not fin(p["voiceGain"][v]) or abs(p["voiceGain"][v]) > 4.0:
            return "voiceGain[%d] must be finite and at most 4 in magnitude" % v
    if not fin(p["feedback"]) or abs(F(p["feedback"])) > F(0.95):
        return "feedback must lie in [-0.95, 0.95]"
    for name in ("wet", "dry"):
        if not fin(p[name]) or abs(p[name]) > 1e6:
            return name + " must be finite and at most 1e6 in magnitude"
    if not fin(p["tremoloDepth"]) or not 0.0 <= p["tremoloDepth"] <= 1.0:
        return "tremoloDepth must lie in [0, 1]"
    return None


def weight(N, k):
    """OutStageWeightAt for an int64 array k: 1 for k >= N - 1, else (float)(k + 1) / (float)N"""
    k = np.asarray(k, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (k + 1).astype(F) / F(max(N, 1))
    return np.where(k >= N - 1, F(1.0), w).astype(F)


def ramp(gA, gB, wk):
    """B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk))"""
    gA, gB = F(gA), F(gB)
    span = F(gB - gA)
    return np.where(wk == F(1.0), gB, (gA + (span * wk).astype(F)).astype(F)).astype(F)


def clamp(v, limit):
    return np.minimum(np.maximum(v, F(-limit)), F(limit)).astype(F)


def x_prime(x):
    x = np.asarray(x, F)
    return np.where(np.isnan(x), F(0.0), clamp(x, 1e18)).astype(F)


def tri_of(u):
    """u: uint64 array of phases modulo 2^32 -> the triangle, exact, in [0, 1)"""
    u = np.asarray(u, np.uint64) & np.uint64(0xFFFFFFFF)
    h = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u)
    return ((h >> np.uint64(7)).astype(F) * F(2.0 ** -24)).astype(F)


def shape_of(shape, tri):
    if shape == TRIANGLE:
        return tri
    square = (tri * tri).astype(F)
    rest = (F(3.0) - (F(2.0) * tri).astype(F)).astype(F)
    return np.minimum((square * rest).astype(F), F(1.0)).astype(F)


def _setting(p):
    """the ten ramped values of a setting; a voice absent from a setting has gain 0 in it"""
    return dict(base=F(p["baseSamples"]), depth=F(p["depthSamples"]), fb=F(p["feedback"]), wet=F(p["wet"]), dry=F(p["dry"]), td=F(p["tremoloDepth"]),
                gain=[F(p["voiceGain"][v]) if v < p["numVoices"] else F(0.0) for v in range(4)])


class ModRef:
    """one stream's modulation: set calls, fades and the line, by the contract"""

    def __init__(self):
        self.has = False

    def remaining(self):
        return self.N - self.k if self.has and self.fading else 0

    def target(self):
        return self.B if self.has and not self.to_none else None

    def set(self, p, N):
        """True: taken; "fade": refused, a fade is running; ("phase", v): refused, voice v sounds and its phase would change"""
        if self.has and self.fading:
            return "fade"
        if not self.has:
            if p is None:
                return True
            self.has, self.to_none, self.fading = True, False, False
            self.B = dict(p)
            self.A = dict(p, wet=0.0, dry=1.0, tremoloDepth=0.0, feedback=0.0)
            self.phase = 0
            self.w = np.zeros(PAD, F)
        else:
            if p is not None:
                for v in range(min(self.B["numVoices"], p["numVoices"])):
                    if self.B["voiceGain"][v] != 0.0 and self.B["voicePhase"][v] != p["voicePhase"][v]:
                        return ("phase", v)
            self.A = self.B
            self.B = dict(p) if p is not None else dict(self.A, wet=0.0, dry=1.0, tremoloDepth=0.0)
            self.to_none = p is None
        self.N, self.k = N, 0
        self.fading = N > 0
        if not self.fading:
            self.A = self.B
            if self.to_none:
                self.has = False
        return True

    def leave(self):
        self.has = False

    def _voices(self, wk, j, line, t0):
        """the taps, m and s_0 of the samples j (int64 array, counted in the call) whose line positions are t0 + j"""
        A, B = _setting(self.A), _setting(self.B)
        base, depth = ramp(A["base"], B["base"], wk), ramp(A["depth"], B["depth"], wk)
        u0 = (np.uint64(self.phase) + (j.astype(np.uint64) * np.uint64(self.B["phaseInc"]))) & np.uint64(0xFFFFFFFF)
        m = tap0 = s0 = None
        for v in range(self.B["numVoices"]):
            tri = tri_of(u0 + np.uint64(self.B["voicePhase"][v]))
            s = shape_of(self.B["shape"], tri)
            if self.A["shape"] != self.B["shape"]:
                sA = shape_of(self.A["shape"], tri)
                blend = (((F(1.0) - wk).astype(F) * sA).astype(F) + (wk * s).astype(F)).astype(F)
                s = np.where(wk == F(1.0), s, blend).astype(F)
            D = (base + (depth * s).astype(F)).astype(F)
            Di = D.astype(np.int32)
            fr = (D - Di.astype(F)).astype(F)
            at = t0 + j - Di
            a, b = line[at], line[at - 1]
            tap = (a + (fr * (b - a).astype(F)).astype(F)).astype(F)
            voice = (ramp(A["gain"][v], B["gain"][v], wk) * tap).astype(F)
            if v == 0:
                m, tap0, s0 = voice, tap, s
            else:
                m = (m + voice).astype(F)
        return m, tap0, s0

    def run(self, x):
        """a processing call: returns what replaces the row's samples (a retired entry leaves the rest of the row as it was)"""
        x = np.asarray(x, F)
        y = x.copy()
        if not self.has or len(x) == 0:
            return y
        n = len(x)
        live = n if not self.to_none else max(0, min(n, self.N - self.k))
        A, B = _setting(self.A), _setting(self.B)
        feeds_back = A["fb"] != 0.0 or B["fb"] != 0.0
        xs = x_prime(x[:live])
        line = np.concatenate([self.w, np.zeros(live, F)])
        t0 = len(self.w)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            runs = [np.arange(live, dtype=np.int64)] if not feeds_back else [np.array([i], np.int64) for i in range(live)]
            if not feeds_back:
                line[t0:] = xs
            for j in runs:
                if len(j) == 0:
                    continue
                k = self.k + j if self.fading else np.full(len(j), 1 << 40, np.int64)
                wk = weight(self.N, k) if self.fading else np.ones(len(j), F)
                m, tap0, s0 = self._voices(wk, j, line, t0)
                fb, wet = ramp(A["fb"], B["fb"], wk), ramp(A["wet"], B["wet"], wk)
                dry, td = ramp(A["dry"], B["dry"], wk), ramp(A["td"], B["td"], wk)
                xj = xs[j]
                if feeds_back:
                    line[t0 + j] = np.where(fb == F(0.0), xj, clamp((xj + (fb * tap0).astype(F)).astype(F), 1e30))
                direct = (dry * xj).astype(F)
                y0 = np.where(wet == F(0.0), direct, (direct + (wet * m).astype(F)).astype(F)).astype(F)
                y[j] = np.where(td == F(0.0), y0, (y0 * (F(1.0) - (td * s0).astype(F)).astype(F)).astype(F))
        self.w = line[-PAD:].copy()
        self.phase = (self.phase + n * self.B["phaseInc"]) & 0xFFFFFFFF
        if self.fading:
            self.k = min(self.N, self.k + n)
            if self.k >= self.N:
                self.fading = False
                self.A = self.B
                if self.to_none:
                    self.has = False
        return y


def run_cuts(p_list, x, cuts):
    """fresh references with settings p_list[row] (None: no entry) over x[rows, total] cut into calls of `cuts` samples"""
    refs = [ModRef() for _ in p_list]
    for ref, p in zip(refs, p_list):
        if p is not None:
            ref.set(p, 0)
    out, pos = [], 0
    for n in cuts:
        out.append(np.stack([ref.run(x[row, pos:pos + n]) for row, ref in enumerate(refs)]))
        pos += n
    return np.concatenate(out, axis=1)


def signal(seed, total, scale=0.5):
    """noise with exact silences, a NaN, infinities and subnormals in it"""
    rng = np.random.default_rng(7300 + seed)
    x = (scale * rng.standard_normal(total)).astype(F)
    x[total // 3:total // 3 + 40] = 0.0
    if total > 64:
        x[17:23] = [np.nan, np.inf, -np.inf, 1e-40, -1e-45, 3e38]
    return x


def chorus(depth=144.0, base=336.0, rate_hz=0.8, shape=SINE, wet=0.7, dry=0.8):
    """three voices a third of a cycle apart, no feedback"""
    return params(base, depth, phase_inc(rate_hz), shape, 3, (0, 0x55555555, 0xAAAAAAAA, 0), None, 0.0, wet, dry)


def flanger(base, depth, fb, rate_hz=37.0, shape=TRIANGLE):
    return params(base, depth, phase_inc(rate_hz), shape, 1, (0, 0, 0, 0), [1.0, 0.0, 0.0, 0.0], fb, 0.7, 0.7)


# the flangers of the issue: (base, depth) -> the kernel's chunk is floor(base) - 1, capped by the group's width
FLANGERS = [(2.0, 3.0), (5.5, 4.25), (48.0, 20.0), (70.0, 30.0), (300.0, 60.0)]
CUTS = [1, 7, 64, 65, 128, PIECE + 1]
