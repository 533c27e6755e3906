"""The SDXL UNet's kernels through the C ABI on both backends (CPU lane emulator / MI355X), against numpy fp64: layernorm16 (K1), geglu16 (K2), the conv16
form for Cout % 64 == 0 (K3) and its per-image channel bias (K4), groupnorm16 with 2 mod 4 channels per group (K5), concat16 (K6), and the shapes that
are still rejected."""
import math

import numpy as np
import pytest

from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi
from test_kernels_vae import bf, conv_ref, f32, frame, u16

SENTINEL = 0x7FC0


def conv_desc(be, XIN, WP, OUT, B, RES, CB, N, H, W, Cin, Ho, Wo, Cout, out_pad, KS, stride, pads, up, in_pad=1):
    return _abi.Conv16Desc(in_=be.ptr(XIN), W=be.ptr(WP), out=be.ptr(OUT), bias=be.ptr(B), residual=be.ptr(RES), N=N, Hi=H, Wi=W, Cin=Cin, in_pad=in_pad,
                           Ho=Ho, Wo=Wo, Cout=Cout, out_pad=out_pad, KS=KS, stride=stride, pad_top=pads[0], pad_left=pads[1], upsample=up, dtype=_abi.DT_BF16,
                           chan_bias=be.ptr(CB))


@pytest.mark.parametrize("case", [
    dict(Cout=64, Cin=192, H=5, W=7),                                      # one 128-wide N tile, half of it masked; partial M tile
    dict(Cout=320, H=4, W=5, res=1),                                       # 2 full N tiles + a masked one, residual
    dict(Cout=960, Cin=128, H=3, W=3, KS=1, res=1),                        # 1 x 1 (the shortcut / proj_out shape), 7.5 N tiles
    dict(Cout=64, H=4, W=4),                                               # weights of 72 KB: the direct kernel, as before ABI 13
    dict(Cout=320, H=3, W=4, up=1),                                        # Upsample2D + conv
    dict(Cout=320, H=6, W=6, stride=2),                                    # Downsample2D: stride 2, padding 1
    dict(Cout=320, H=4, W=4, cb=1),                                        # K4: per-image channel bias alone
    dict(Cout=320, H=5, W=3, cb=1, res=1),                                 # K4 with a residual
    dict(Cout=128, H=5, W=3, cb=1, res=1),                                 # K4 on a Cout % 128 == 0 layer (the UNet form takes it)
])
def test_conv16_unet_forms(be, case):
    rng = np.random.default_rng(case["Cout"] + 7 * case["H"] + case.get("cb", 0))
    Cin, Cout, H, W = case.get("Cin", 64), case["Cout"], case["H"], case["W"]
    KS, stride, up = case.get("KS", 3), case.get("stride", 1), case.get("up", 0)
    N = 2
    x, w, b = bf(rng.standard_normal((N, Cin, H, W))), bf(rng.standard_normal((Cout, Cin, KS, KS)) / (Cin * KS * KS) ** 0.5), bf(rng.standard_normal(Cout))
    if up:
        ref, pads = conv_ref(x, w, b, up=True), (1, 1)
    elif stride == 2:
        ref, pads = conv_ref(x, w, b, stride=2, pads=(1, 1, 1, 1)), (1, 1)
    else:
        p = (KS - 1) // 2
        ref, pads = conv_ref(x, w, b, pads=(p, p, p, p)), (p, p)
    Ho, Wo = ref.shape[2], ref.shape[3]
    res = bf(rng.standard_normal((N, Cout, Ho, Wo))) if case.get("res") else None
    cb = bf(rng.standard_normal((N, Cout))) if case.get("cb") else None
    if cb is not None:
        ref = ref + cb[:, :, None, None]
    if res is not None:
        ref = ref + res
    # the weight buffer is followed by sentinel rows that a read of rows >= Cout would pick up (NaN in bf16)
    wp = np.full((Cout + 128, KS * KS, Cin), SENTINEL, np.uint16)
    wp[:Cout] = u16(w.transpose(0, 2, 3, 1).reshape(Cout, KS * KS, Cin))
    XIN, WP, B = be.dev(frame(x, 1)), be.dev(wp), be.dev(u16(b))
    OUT = be.dev(np.full((N, Ho + 2, Wo + 2, Cout), SENTINEL, np.uint16))
    RES = be.dev(frame(res, 1)) if res is not None else None
    CB = be.dev(u16(cb)) if cb is not None else None
    ok(be.lib.eegclip_conv16(conv_desc(be, XIN, WP, OUT, B, RES, CB, N, H, W, Cin, Ho, Wo, Cout, 1, KS, stride, pads, up), be.stream))
    be.sync()
    got = be.host(OUT)
    inner = f32(got[:, 1:1 + Ho, 1:1 + Wo, :]).transpose(0, 3, 1, 2)
    assert np.isfinite(inner).all()
    np.testing.assert_allclose(inner, ref, atol=8e-3 * max(1.0, np.abs(ref).max()))
    assert (got[:, 0] == SENTINEL).all() and (got[:, -1] == SENTINEL).all() and (got[:, :, 0] == SENTINEL).all() and (got[:, :, -1] == SENTINEL).all()


def test_conv16_rejects(be):
    N, H, W = 1, 4, 4
    XIN, WP = be.dev(np.zeros((N, H + 2, W + 2, 64), np.uint16)), be.dev(np.zeros((96, 9, 64), np.uint16))
    OUT = be.dev(np.zeros((N, H + 2, W + 2, 96), np.uint16))
    CB = be.dev(np.zeros((N, 96), np.uint16))
    # Cout % 64 != 0 with Cin % 64 == 0: weights (96 x 9 x 64 x 2 = 108 KB) fit the direct kernel, but a channel bias is an epilogue of the matrix forms only
    assert be.lib.eegclip_conv16(conv_desc(be, XIN, WP, OUT, None, None, CB, N, H, W, 64, H, W, 96, 1, 3, 1, (1, 1), 0), be.stream) < 0
    # a 320-channel 3 x 3 layer with Cin % 64 != 0 has no matrix form and is too large for the direct one
    XIN2, WP2 = be.dev(np.zeros((N, H + 2, W + 2, 96), np.uint16)), be.dev(np.zeros((320, 9, 96), np.uint16))
    OUT2 = be.dev(np.zeros((N, H + 2, W + 2, 320), np.uint16))
    assert be.lib.eegclip_conv16(conv_desc(be, XIN2, WP2, OUT2, None, None, None, N, H, W, 96, H, W, 320, 1, 3, 1, (1, 1), 0), be.stream) < 0


@pytest.mark.parametrize("C", [320, 640, 960, 1280, 2560])
def test_groupnorm16_unet_channel_counts(be, C):
    """32 groups of 10 / 20 / 30 / 40 / 80 channels: the fixed-order statistics form (+ the 2-channel apply for 10 / 30); two passes are bit-identical"""
    rng = np.random.default_rng(C)
    N, H, W, G = 2, 3, 5, 32
    x = bf(rng.standard_normal((N, C, H, W)) * 2 + 0.5)
    g, b = bf(1 + 0.2 * rng.standard_normal(C)), bf(0.2 * rng.standard_normal(C))
    X, GA, BE = be.dev(frame(x, 1)), be.dev(u16(g)), be.dev(u16(b))
    for silu in (0, 1):
        Y, S = be.dev(np.zeros((N, H + 2, W + 2, C), np.uint16)), be.dev(np.full(N * G * 2, np.nan, np.float64))
        ok(be.lib.eegclip_groupnorm16(be.ptr(X), N, H, W, C, 1, G, be.ptr(GA), be.ptr(BE), 1e-5, silu, be.ptr(Y), 1, be.ptr(S), _abi.DT_BF16, be.stream))
        be.sync()
        y1, s1 = be.host(Y).copy(), be.host(S).copy()
        ok(be.lib.eegclip_groupnorm16(be.ptr(X), N, H, W, C, 1, G, be.ptr(GA), be.ptr(BE), 1e-5, silu, be.ptr(Y), 1, be.ptr(S), _abi.DT_BF16, be.stream))
        be.sync()
        assert np.array_equal(be.host(S), s1) and np.array_equal(be.host(Y), y1)             # fixed summation order
        xg = x.astype(np.float64).reshape(N, G, -1)
        ref = ((xg - xg.mean(2, keepdims=True)) / np.sqrt(xg.var(2, keepdims=True) + 1e-5)).reshape(N, C, H, W) * g[None, :, None, None] + b[None, :, None, None]
        if silu:
            ref = ref / (1 + np.exp(-ref))
        got = be.host(Y)
        np.testing.assert_allclose(f32(got[:, 1:-1, 1:-1, :]).transpose(0, 3, 1, 2), ref, atol=2e-2)
        assert not got[:, 0].any() and not got[:, :, -1].any()
    # odd channels per group (64 groups of 320 / 960: 5 / 15; 320 groups of 2560 - 2 mod 4 fine, but 2560 / 512 = 5) are still rejected
    Y = be.dev(np.zeros((N, H + 2, W + 2, C), np.uint16))
    S = be.dev(np.zeros(N * 512 * 2, np.float64))
    odd = next(g for g in (64, 128, 256, 512) if C % g == 0 and (C // g) % 2)
    assert be.lib.eegclip_groupnorm16(be.ptr(X), N, H, W, C, 1, odd, be.ptr(GA), be.ptr(BE), 1e-5, 0, be.ptr(Y), 1, be.ptr(S), _abi.DT_BF16, be.stream) < 0


@pytest.mark.parametrize("C", [320, 640, 1280])
def test_layernorm16(be, C):
    rng = np.random.default_rng(C)
    rows, ld = 7, C + 64
    x = bf(rng.standard_normal((rows, C)) * 3 + 1.0)
    g, b = bf(1 + 0.3 * rng.standard_normal(C)), bf(0.3 * rng.standard_normal(C))
    xs = np.zeros((rows, ld), np.uint16)
    xs[:, :C] = u16(x)
    X, GA, BE = be.dev(xs), be.dev(u16(g)), be.dev(u16(b))
    Y = be.dev(np.full((rows, C), SENTINEL, np.uint16))
    ok(be.lib.eegclip_layernorm16(be.ptr(X), ld, be.ptr(GA), be.ptr(BE), be.ptr(Y), C, rows, C, 1e-5, _abi.DT_BF16, be.stream))
    be.sync()
    xd = x.astype(np.float64)
    ref = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-5) * g + b
    np.testing.assert_allclose(f32(be.host(Y)), ref, atol=3e-2, rtol=1e-2)
    assert be.lib.eegclip_layernorm16(be.ptr(X), ld, be.ptr(GA), be.ptr(BE), be.ptr(Y), C, rows, C - 4, 1e-5, _abi.DT_BF16, be.stream) < 0     # C % 8
    assert be.lib.eegclip_layernorm16(be.ptr(X), ld, be.ptr(GA), be.ptr(BE), be.ptr(Y), C, rows, 8192, 1e-5, _abi.DT_BF16, be.stream) < 0       # C > 4096


def h16(x):
    return np.ascontiguousarray(x, np.float16).view(np.uint16)


@pytest.mark.parametrize("C", [64, 320, 1280])
def test_layernorm16_fp16_against_fp64(be, C):
    """fp16 against fp64 within one fp16 ulp of the exact value, plus 6e-5 of the summands' size |(x - mean) rstd gamma| + |beta| (fp32 arithmetic: in the
    low-variance rows the rounded mean alone moves the normalised value by ~1e-5 of itself, many ulps of a result that gamma and beta nearly cancel).
    The biased variance (an unbiased one moves every value by C / (C - 1): 1.6 % at C = 64, 0.16 % at 320, i.e. 1.5 ulp at |value| ~ 2) and eps inside
    the square root (rows of variance ~1e-5: eps 1e-5 moves them by ~30 %) both count"""
    rng = np.random.default_rng(C + 1)
    rows = 6
    scale = np.where(np.arange(rows) % 2 == 0, 2.0, 3e-3)[:, None]            # every other row: variance ~1e-5, where eps matters
    x = (rng.standard_normal((rows, C)) * scale + 0.5).astype(np.float16)
    g, b = (1 + 0.3 * rng.standard_normal(C)).astype(np.float16), (0.3 * rng.standard_normal(C)).astype(np.float16)
    X, GA, BE = be.dev(h16(x)), be.dev(h16(g)), be.dev(h16(b))
    Y = be.dev(np.full((rows, C), SENTINEL, np.uint16))
    ok(be.lib.eegclip_layernorm16(be.ptr(X), C, be.ptr(GA), be.ptr(BE), be.ptr(Y), C, rows, C, 1e-5, _abi.DT_F16, be.stream))
    be.sync()
    got = be.host(Y).view(np.float16).astype(np.float64)
    xd = x.astype(np.float64)
    ng = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-5) * g.astype(np.float64)
    ref = ng + b.astype(np.float64)
    bound = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64) + 6e-5 * (np.abs(ng) + np.abs(b.astype(np.float64)))
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())


def test_geglu16(be):
    rng = np.random.default_rng(3)
    M, D = 5, 320 * 4
    x = bf(rng.standard_normal((M, 2 * D)) * 2)
    X, Y = be.dev(u16(x)), be.dev(np.full((M, D), SENTINEL, np.uint16))
    ok(be.lib.eegclip_geglu16(be.ptr(X), be.ptr(Y), M, D, _abi.DT_BF16, be.stream))
    be.sync()
    a, g = x[:, :D].astype(np.float64), x[:, D:].astype(np.float64)
    erf = np.vectorize(math.erf)
    ref = a * 0.5 * g * (1 + erf(g / math.sqrt(2)))
    np.testing.assert_allclose(f32(be.host(Y)), ref, atol=2e-2, rtol=1e-2)
    assert be.lib.eegclip_geglu16(be.ptr(X), be.ptr(Y), M, 12, _abi.DT_BF16, be.stream) < 0                    # D % 8


def test_concat16(be):
    rng = np.random.default_rng(4)
    N, H, W, Ca, Cb = 2, 3, 4, 64, 320
    a, b = bf(rng.standard_normal((N, Ca, H, W))), bf(rng.standard_normal((N, Cb, H, W)))
    A, B = be.dev(frame(a, 1)), be.dev(frame(b, 1))
    OUT = be.dev(np.full((N, H + 2, W + 2, Ca + Cb), SENTINEL, np.uint16))
    ok(be.lib.eegclip_concat16(be.ptr(A), be.ptr(B), be.ptr(OUT), N, H, W, 1, Ca, Cb, 1, _abi.DT_BF16, be.stream))
    be.sync()
    got = be.host(OUT)
    np.testing.assert_array_equal(f32(got[:, 1:-1, 1:-1, :]).transpose(0, 3, 1, 2), np.concatenate([a, b], 1))
    assert (got[:, 0] == SENTINEL).all() and (got[:, -1] == SENTINEL).all() and (got[:, :, 0] == SENTINEL).all() and (got[:, :, -1] == SENTINEL).all()
    assert be.lib.eegclip_concat16(be.ptr(A), be.ptr(B), be.ptr(OUT), N, H, W, 1, Ca, 12, 1, _abi.DT_BF16, be.stream) < 0                 # Cb % 8
