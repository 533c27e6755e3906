"""csrc/metric_nets.hip through the C ABI on both backends (CPU lane emulator / MI355X): eegclip_convrelu16 on torchvision AlexNet's five layer shapes,
eegclip_maxpool16 and eegclip_pack_nchw16, against tests/metric_nets_ref.py (fp64 torch.nn.functional on the CPU).

Operands are values exact in the 16-bit dtype and the reference is fp64 of those same values, so the bound has two terms and no slack:
    |y - ref| <= u |ref| + K 2^-23 (|x| (*) |w|)
u = 2^-11 (fp16) / 2^-8 (bf16): the one rounding at the store; K = KS^2 Cin terms accumulated in fp32, |x| (*) |w| the convolution of the absolute values.  The one-hot probes are exact: they are what a swapped ky / kx, a wrong
stride or a wrong padding cannot pass at a tolerance."""
import numpy as np
import pytest
import torch

import metric_nets_ref as R
from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi

DT = {torch.float16: _abi.DT_F16, torch.bfloat16: _abi.DT_BF16}
LAYER = {i: (cin, cout, k, s, p) for i, cin, cout, k, s, p in R.LAYERS}
NEXT_PAD = {"0": 0, "3": 0, "6": 1, "8": 1, "10": 0}       # the border of each layer's output frame in the net (a pool reads unpadded frames)


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def launch(be, i, x, w, b, dtype, out_pad, via_pack=False):
    """features.i on x (N, Cin, H, W), all operands exact in dtype -> (output frame patterns, Ho, Wo)"""
    cin, cout, k, s, p = LAYER[i]
    N, _, H, W = x.shape
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    if cin == 3:
        width = be.lib.eegclip_convrelu16_in_width(W)
        assert width % 2 == 0 and width >= max(W + 4, 4 * (Wo - 1) + 16)
        host = R.first_frame(x, width, dtype)
        if via_pack:                                          # the pack kernel writes the interior of a zero frame: the frame the restatement builds
            XIN, PLANES = be.dev(np.zeros_like(host)), be.dev(R.bits(x, dtype))
            ok(be.lib.eegclip_pack_nchw16(be.ptr(PLANES), be.ptr(XIN), N, H, W, DT[dtype], be.stream))
            be.sync()
            assert np.array_equal(be.host(XIN), host)
        else:
            XIN = be.dev(host)
    else:
        XIN = be.dev(R.frame(x, p, dtype))
    WP, B = be.dev(R.pack_weight(w, dtype)), be.dev(R.bits(b, dtype))
    OUT = be.dev(np.zeros((N, Ho + 2 * out_pad, Wo + 2 * out_pad, cout), np.uint16))
    d = _abi.ConvRelu16Desc(in_=be.ptr(XIN), W=be.ptr(WP), bias=be.ptr(B), out=be.ptr(OUT), N=N, Hi=H, Wi=W, Cin=cin, Cout=cout, KS=k, stride=s, pad=p,
                            out_pad=out_pad, dtype=DT[dtype])
    ok(be.lib.eegclip_convrelu16(d, be.stream))
    be.sync()
    return be.host(OUT), Ho, Wo


def operands(i, N, H, W, dtype, seed):
    cin, cout, k, s, p = LAYER[i]
    g = torch.Generator().manual_seed(seed)
    x = R.exact(torch.randn(N, cin, H, W, generator=g), dtype)
    w = R.exact(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, dtype)
    b = R.exact(0.5 * torch.randn(cout, generator=g), dtype)
    return x, w, b


CASES = [("0", 31, 37), ("3", 3, 4), ("3", 7, 9), ("6", 3, 4), ("8", 3, 4), ("10", 3, 4)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("i,H,W", CASES, ids=[f"features.{i}-{H}x{W}" for i, H, W in CASES])
def test_convrelu16_against_fp64(be, i, H, W, dtype):
    """N = 2.  features.0 on 31 x 37 -> 7 x 8: both borders take part, (W + 4 - 11) % 4 = 2 leaves the two rightmost frame columns outside every window, M = 112
    is a tile tail; features.3's Cout = 192 is three 64-wide N tiles; 7 x 9 gives M = 126."""
    cin, cout, k, s, p = LAYER[i]
    x, w, b = operands(i, 2, H, W, dtype, 100 + int(i) + H)
    out_pad = NEXT_PAD[i] if i != "3" or H == 3 else 2       # (features.3 at 7 x 9 also with the widest border a frame takes)
    got, Ho, Wo = launch(be, i, x, w, b, dtype, out_pad, via_pack=True)
    ref = R.conv_relu(x, w, b, s, p)
    assert tuple(ref.shape) == (2, cout, Ho, Wo)
    if i == "0":
        assert (Ho, Wo) == (7, 8) and 2 * Ho * Wo == 112
    y = R.unframe(got, out_pad, dtype)
    bound = R.UNIT[dtype] * ref.abs() + cin * k * k * 2.0 ** -23 * R.conv_abs(x, w, s, p)
    err = (y - ref).abs()
    print(f"\n[metric_nets] features.{i} {H}x{W} {dtype}: max err {float(err.max()):.2e}, max err / bound {float((err / bound).max()):.3f}", end=" ")
    assert bool((err <= bound).all())
    assert R.border_is_zero(got, out_pad)
    assert float((ref == 0).double().mean()) > 0.2 and float((ref > 0).double().mean()) > 0.2       # the ReLU is exercised on both sides


def probe_hits(k, s, p, H, W, ky, kx, py, px):
    """output positions whose window holds input pixel (py, px) at tap (ky, kx): y s + ky - p == py, x s + kx - p == px"""
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    return [(y, x) for y in range(Ho) for x in range(Wo) if y * s + ky - p == py and x * s + kx - p == px]


def probes(i, H, W):
    """two probes per layer: the last tap (KS - 1, KS - 1) with the input pixel nearest the last row / column that it reaches, and the pixel in the last row
    and column with an off-diagonal tap (ky != kx) that reaches it; channels at both ends"""
    cin, cout, k, s, p = LAYER[i]
    a = next((py, px) for py in range(H - 1, -1, -1) for px in range(W - 1, -1, -1) if probe_hits(k, s, p, H, W, k - 1, k - 1, py, px))
    t = next((ky, kx) for kx in range(k - 1, -1, -1) for ky in range(k - 1, -1, -1) if ky != kx and probe_hits(k, s, p, H, W, ky, kx, H - 1, W - 1))
    return [dict(co=cout - 1, ky=k - 1, kx=k - 1, ci=cin - 1, py=a[0], px=a[1], n=1), dict(co=0, ky=t[0], kx=t[1], ci=0, py=H - 1, px=W - 1, n=0)]


@pytest.mark.parametrize("i,H,W", [("0", 31, 37), ("3", 3, 4), ("6", 3, 4), ("8", 3, 4), ("10", 3, 4)], ids=lambda v: str(v))
def test_convrelu16_one_hot_probes(be, i, H, W):
    """one input element and one weight element are 1, the rest 0: the output is exactly 1 where the definition puts that tap on that pixel and exactly
    relu(bias) everywhere else (the bias of the probed channel is 0, the others are random of both signs)"""
    cin, cout, k, s, p = LAYER[i]
    dtype = torch.float16
    for pr in probes(i, H, W):
        x, w = torch.zeros(2, cin, H, W, dtype=torch.float64), torch.zeros(cout, cin, k, k, dtype=torch.float64)
        x[pr["n"], pr["ci"], pr["py"], pr["px"]] = 1.0
        w[pr["co"], pr["ci"], pr["ky"], pr["kx"]] = 1.0
        b = R.exact(torch.randn(cout, generator=torch.Generator().manual_seed(7)), dtype)
        b[pr["co"]] = 0.0
        hits = probe_hits(k, s, p, H, W, pr["ky"], pr["kx"], pr["py"], pr["px"])
        assert hits
        got, Ho, Wo = launch(be, i, x, w, b, dtype, NEXT_PAD[i])
        want = torch.relu(b)[None, :, None, None].expand(2, cout, Ho, Wo).clone()
        for y, xx in hits:
            want[pr["n"], pr["co"], y, xx] = 1.0
        assert torch.equal(R.unframe(got, NEXT_PAD[i], dtype), want), pr
        assert torch.equal(want, R.conv_relu(x, w, b, s, p))          # (the definition used here is torch's)
        assert R.border_is_zero(got, NEXT_PAD[i])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_convrelu16_negative_bias_stores_zero(be, dtype):
    """zero input, a negative bias everywhere: every stored pattern is +0"""
    for i, H, W in (("0", 15, 16), ("3", 3, 4)):
        cin, cout, k, s, p = LAYER[i]
        _, w, _ = operands(i, 1, H, W, dtype, 3)
        got, _, _ = launch(be, i, torch.zeros(1, cin, H, W, dtype=torch.float64), w, R.exact(-0.1 - torch.rand(cout), dtype), dtype, 1)
        assert not got.any()


@pytest.mark.parametrize("C,in_pad,out_pad", [(64, 0, 2), (192, 0, 1), (64, 1, 0), (192, 2, 2)])
@pytest.mark.parametrize("H,W", [(7, 8), (9, 7)])
def test_maxpool16_negative_input_bit_exact(be, H, W, C, in_pad, out_pad):
    """7 -> 3, 8 -> 3 and 9 -> 4 with every input negative (a maximum that started from 0, or a tap in the input frame's zero border, would store 0): the
    patterns are the reference's, the border stays 0"""
    for dtype in (torch.float16, torch.bfloat16):
        x = R.exact(-0.05 - torch.rand(2, C, H, W, generator=torch.Generator().manual_seed(H * W + C)) * 4, dtype)
        ref = torch.nn.functional.max_pool2d(x, 3, 2)
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        assert tuple(ref.shape) == (2, C, Ho, Wo) and {7: 3, 8: 3, 9: 4}[H] == Ho and {7: 3, 8: 3, 9: 4}[W] == Wo and bool((ref < 0).all())
        XIN, OUT = be.dev(R.frame(x, in_pad, dtype)), be.dev(np.zeros((2, Ho + 2 * out_pad, Wo + 2 * out_pad, C), np.uint16))
        ok(be.lib.eegclip_maxpool16(be.ptr(XIN), be.ptr(OUT), 2, H, W, C, in_pad, out_pad, DT[dtype], be.stream))
        be.sync()
        got = be.host(OUT)
        assert np.array_equal(got, R.frame(ref, out_pad, dtype))
        assert R.border_is_zero(got, out_pad)


def test_refusals(be):
    """anything but AlexNet's five layers, a bad frame padding, or a pool the kernel does not take: EEGCLIP_EINVAL, nothing launched"""
    buf = be.dev(np.zeros(1 << 16, np.uint16))
    good = dict(in_=be.ptr(buf), W=be.ptr(buf), bias=be.ptr(buf), out=be.ptr(buf), N=1, Hi=3, Wi=3, Cin=64, Cout=192, KS=5, stride=1, pad=2, out_pad=0,
                dtype=_abi.DT_F16)
    for change in (dict(KS=7), dict(KS=3), dict(stride=2), dict(pad=1), dict(Cin=128), dict(Cout=128), dict(Cin=3), dict(out_pad=3), dict(N=0), dict(dtype=_abi.DT_F32),
                   dict(bias=None), dict(Cin=3, Cout=64, KS=11, stride=4, pad=2, Hi=6, Wi=31), dict(Cin=64, Cout=64, KS=3, pad=1)):
        assert be.lib.eegclip_convrelu16(_abi.ConvRelu16Desc(**{**good, **change}), be.stream) == -1, change
    assert be.lib.eegclip_convrelu16_in_width(6) == -1
    for args in ((1, 2, 8, 64, 0, 0), (1, 8, 8, 60, 0, 0), (1, 8, 8, 64, 3, 0), (1, 8, 8, 64, 0, 3), (0, 8, 8, 64, 0, 0)):
        assert be.lib.eegclip_maxpool16(be.ptr(buf), be.ptr(buf), *args, _abi.DT_F16, be.stream) == -1, args
    assert be.lib.eegclip_maxpool16(be.ptr(buf), be.ptr(buf), 1, 8, 8, 64, 0, 0, _abi.DT_F32, be.stream) == -1
    assert be.lib.eegclip_pack_nchw16(be.ptr(buf), be.ptr(buf), 1, 6, 31, _abi.DT_F16, be.stream) == -1
