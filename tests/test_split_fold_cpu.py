"""Folded operands of the f16-split kernels (WN_FLAG_FOLD, wavenet_plan.cpp FillSplitFoldAux), host side only: the A-operand image of every
folded layer, multiplied out in numpy as the k-sums of the MFMA sequence the kernels issue, gives exactly the three-product split of
conv + mix-in + bias and of 1x1 + bias -- the products of the unfolded layout, only summed in fewer MFMAs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import na_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")
WN_ST_LAYER, WN_FLAG_FOLD = 1, 32


@pytest.fixture(scope="module")
def na():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "neuralaudio_amd", "libNeuralAudioCAPI.so")):
        g.build()
    import neuralaudio_amd
    return neuralaudio_amd


def _split_plan(na, name):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = na.NeuralModelLoader().CreateFromFile(os.path.join(MODELS, name), doPrewarm=False)
    count = C.c_longlong(0)
    n = lib.NA_DebugSplitPlan(m._h, None, 0, None, 0, C.byref(count))
    assert n > 0, capi.last_error()
    stages = np.zeros((n, 16), np.int32)
    wsplit = np.zeros(count.value, np.uint16)
    assert lib.NA_DebugSplitPlan(m._h, stages.ctypes.data_as(C.POINTER(C.c_int)), n, wsplit.ctypes.data_as(C.POINTER(C.c_ushort)),
                                 count.value, C.byref(count)) == n
    return stages, wsplit.view(np.float16).astype(np.float64)


def _split(v):
    h = v.astype(np.float16)
    return h.astype(np.float64), (v - h.astype(np.float32)).astype(np.float16).astype(np.float64)


def _quads(v, Gp, second):
    """B operand of the 4 k-blocks (lane k-block q = tile slot q // Gp, channel group q % Gp): [h(4) | second(4)], second = 'l' or 'c8'."""
    h, l = _split(v)
    out = np.zeros((4, 8))
    for q in range(4):
        cg = q % Gp
        out[q, :4] = h[4 * cg:4 * cg + 4] if 4 * cg < len(v) else 0.0
        if isinstance(second, str):
            out[q, 4:] = l[4 * cg:4 * cg + 4] if 4 * cg < len(v) else 0.0
        else:
            out[q, 4:] = second
    return out


def _h_pair(a, b, Gp):
    ha, _ = _split(a)
    hb, _ = _split(b)
    out = np.zeros((4, 8))
    for q in range(4):
        cg = q % Gp
        out[q, :4], out[q, 4:] = ha[4 * cg:4 * cg + 4], hb[4 * cg:4 * cg + 4]
    return out


def _mfma(image, op, B):
    """D[row] = sum over k-blocks q and slots r of A[lane q*16 + row][r] * B[q][r] (one frame column)."""
    A = image[op * 512:(op + 1) * 512].reshape(4, 16, 8)
    return np.einsum("qor,qr->o", A, B)


def test_standard_layers_are_folded_and_multiply_out_to_the_split_products(na):
    stages, image = _split_plan(na, "BossWN-standard.nam")
    j = O.load_json("BossWN-standard.nam")
    arrays = O.wavenet_arrays_from_nam(j)
    w = np.asarray(j["weights"], np.float32)
    tens = {(nm, a, l): w[sl] for nm, a, l, sl in O.wavenet_tensor_slices(arrays)}
    layers = [(a, l) for a, arr in enumerate(arrays) for l in range(len(arr["kernel_sizes"]))]
    ls = stages[stages[:, 0] == WN_ST_LAYER]
    assert len(ls) == len(layers) == 20
    rng = np.random.default_rng(7)
    for st, (a, l) in zip(ls, layers):
        Cn, K, Gp, a_off, a_ops = arrays[a]["channels"], 3, int(st[3]), int(st[13]), int(st[14])
        assert st[1] & WN_FLAG_FOLD and st[4] == K and a_ops == 2 * K + 4
        op0 = a_off // 64
        conv = tens[("conv", a, l)].reshape(Cn, Cn, K)
        bconv, mix = tens[("conv_bias", a, l)], tens[("mixin", a, l)]
        w1, b1 = tens[("1x1", a, l)].reshape(Cn, Cn), tens[("1x1_bias", a, l)]
        for unused in (3, 6, 9):
            assert not image[(op0 + unused) * 512:(op0 + unused + 1) * 512].any()
        for _ in range(4):
            x = [rng.uniform(-2, 2, Cn).astype(np.float32) for _ in range(K)]
            z = rng.uniform(-1, 1, Cn).astype(np.float32)
            cond = np.float32(rng.uniform(-1, 1))
            ch = np.float64(np.float16(cond))
            cl = np.float64(np.float16(cond - np.float32(ch)))
            c8 = np.array([ch, 1.0, cl, 1.0])
            # the kernels' sequence: hi tap 0, hi tap 1, [Wl_0 | Wl_1], hi tap 2, [Wl_2 | aux]; 1x1 hi, [W1l | b1]
            d = (_mfma(image, op0, _quads(x[0], Gp, "l")) + _mfma(image, op0 + 2, _quads(x[1], Gp, "l"))
                 + _mfma(image, op0 + 1, _h_pair(x[0], x[1], Gp)) + _mfma(image, op0 + 4, _quads(x[2], Gp, "l"))
                 + _mfma(image, op0 + 5, _quads(x[2], Gp, c8)))
            y = _mfma(image, op0 + 7, _quads(z, Gp, "l")) + _mfma(image, op0 + 8, _quads(z, Gp, c8))
            # expected: the three-product split of every product, in float64
            exp = np.zeros(Cn)
            for k in range(K):
                wh, wl = _split(conv[:, :, k])
                xh, xl = _split(x[k])
                exp += wh @ xh + wh @ xl + wl @ xh
            mh, ml = _split(mix.reshape(Cn))
            bh, bl = _split(bconv)
            exp += mh * ch + bh + mh * cl + bl + ml * ch
            w1h, w1l = _split(w1)
            zh, zl = _split(z)
            b1h, b1l = _split(b1)
            exp1 = w1h @ zh + w1h @ zl + w1l @ zh + b1h + b1l
            for p in range(4 // Gp):  # every tile slot holds the same rows
                rows = slice(4 * Gp * p, 4 * Gp * p + Cn)
                np.testing.assert_allclose(d[rows], exp, rtol=0, atol=1e-12)
                np.testing.assert_allclose(y[rows], exp1, rtol=0, atol=1e-12)
            # and that is the layer's f32 arithmetic to within the split's rounding
            ref = sum(conv[:, :, k].astype(np.float64) @ x[k] for k in range(K)) + mix.reshape(Cn) * np.float64(cond) + bconv
            np.testing.assert_allclose(d[:Cn], ref, rtol=0, atol=1e-5 * (1 + np.abs(ref).max()))

