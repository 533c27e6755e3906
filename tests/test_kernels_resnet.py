"""csrc/metric_nets.hip's ResNet entry points through the C ABI on both backends (CPU lane emulator / MI355X): eegclip_convbn16, eegclip_pack_nchw16_stem,
eegclip_maxpool16_pad, eegclip_avgpool16 and eegclip_corr_distance, against tests/resnet_ref.py (fp64 torch.nn.functional and scipy on the CPU).

Convolution operands (input, weights, residual) are values exact in the 16-bit dtype, scale and shift are fp32, and the reference is fp64 of those same
values, so the bound is tests/test_kernels_metric_nets.py's with the epilogue's terms:
    |y - ref| <= u |ref| + tiny + (K + 4) 2^-23 (|scale| (|x| (*) |w|) + |shift| + |residual|)
u = 2^-11 (fp16) / 2^-8 (bf16): the one rounding at the store; tiny = 2^-25 in fp16 (half the spacing of its subnormals: without the ReLU a sum can land
there), 0 in bf16; K = KS^2 Cin terms accumulated in fp32 and four more fp32 roundings (the product with scale, the two sums, and the sum's own carry)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metric_nets_ref as MR
import resnet_ref as R
from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi

DT = {torch.float16: _abi.DT_F16, torch.bfloat16: _abi.DT_BF16}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def launch(be, x, w, scale, shift, stride, pad, dtype, out_pad, relu, residual=None, via_pack=False):
    """one eegclip_convbn16 launch on x (N, Cin, H, W) -> (output frame patterns, Ho, Wo); the output frame starts as zeros"""
    N, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    if cin == 3:
        width = be.lib.eegclip_convbn16_in_width(W)
        assert width % 2 == 0 and width >= max(W + 6, 2 * (Wo - 1) + 16)
        host = R.stem_frame(x, width, dtype)
        if via_pack:
            XIN, PLANES = be.dev(np.zeros_like(host)), be.dev(MR.bits(x, dtype))
            ok(be.lib.eegclip_pack_nchw16_stem(be.ptr(PLANES), be.ptr(XIN), N, H, W, DT[dtype], be.stream))
            be.sync()
            assert np.array_equal(be.host(XIN), host)
        else:
            XIN = be.dev(host)
    else:
        XIN = be.dev(MR.frame(x, pad, dtype))
    WP = be.dev(MR.pack_weight(w, dtype))
    SC, SH = be.dev(scale.float().numpy()), be.dev(shift.float().numpy())
    RES = be.dev(MR.frame(residual, out_pad, dtype)) if residual is not None else None
    OUT = be.dev(np.zeros((N, Ho + 2 * out_pad, Wo + 2 * out_pad, cout), np.uint16))
    d = _abi.ConvBn16Desc(in_=be.ptr(XIN), W=be.ptr(WP), scale=be.ptr(SC), shift=be.ptr(SH), residual=be.ptr(RES), out=be.ptr(OUT), N=N, Hi=H, Wi=W, Cin=cin,
                          Cout=cout, KS=k, stride=stride, pad=pad, out_pad=out_pad, relu=int(relu), dtype=DT[dtype])
    ok(be.lib.eegclip_convbn16(d, be.stream))
    be.sync()
    return be.host(OUT), Ho, Wo


def operands(N, cin, cout, k, stride, H, W, dtype, seed, with_res):
    g = torch.Generator().manual_seed(seed)
    x = MR.exact(torch.randn(N, cin, H, W, generator=g), dtype)
    w = MR.exact(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, dtype)
    scale = ((0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.5, -1.0, 1.0)).float()      # both signs
    shift = (0.5 * torch.randn(cout, generator=g)).float()
    Ho, Wo = out_size(H, k, stride, k // 2 if cin != 3 else 3), out_size(W, k, stride, k // 2 if cin != 3 else 3)
    res = MR.exact(torch.randn(N, cout, Ho, Wo, generator=g), dtype) if with_res else None
    return x, w, scale, shift, res


def check_launch(be, x, w, scale, shift, res, stride, pad, dtype, out_pad, relu, label, via_pack=False):
    cout, cin, k, _ = w.shape
    got, Ho, Wo = launch(be, x, w, scale, shift, stride, pad, dtype, out_pad, relu, res, via_pack)
    ref = R.conv_bn(x, w, scale, shift, stride, pad, res, relu)
    assert tuple(ref.shape) == (x.shape[0], cout, Ho, Wo)
    y = MR.unframe(got, out_pad, dtype)
    mag = scale.double().abs()[None, :, None, None] * R.conv_abs(x, w, stride, pad) + shift.double().abs()[None, :, None, None]
    if res is not None:
        mag = mag + res.double().abs()
    bound = R.UNIT[dtype] * ref.abs() + TINY[dtype] + (cin * k * k + 4) * 2.0 ** -23 * mag
    err = (y - ref).abs()
    print(f"\n[resnet] {label} {dtype}: max err {float(err.max()):.2e}, max err / bound {float((err / bound).max()):.3f}", end=" ")
    assert bool((err <= bound).all())
    assert MR.border_is_zero(got, out_pad)
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    if relu:
        assert float((ref == 0).double().mean()) > 0.2 and float((ref > 0).double().mean()) > 0.2
    else:
        assert float((ref < 0).double().mean()) > 0.2


# (KS, stride, Cin, Cout, H, W, out_pad, residual, relu), N = 2
CASES = [(1, 1, 64, 64, 9, 11, 0, False, True),          # one k-tile, the 64-wide N tile, M = 198: two M tiles, the second a tail
         (1, 2, 128, 256, 9, 11, 1, True, False),        # the downsample's shape: (9 - 1) / 2 + 1 = 5, (11 - 1) / 2 + 1 = 6; two k-tiles; no ReLU: negative outputs
         (1, 2, 64, 64, 8, 10, 0, False, False),         # even sizes: the last row and column are never read
         (3, 1, 64, 256, 9, 11, 1, True, True),          # conv3-like epilogue on a 3 x 3 layer: every border tap
         (3, 2, 128, 64, 9, 11, 0, False, True),         # conv2 with the stride: the bottom / right border taps of odd sizes
         (3, 2, 64, 128, 8, 10, 1, True, True),          # even sizes: the bottom / right padding row is never read
         (3, 1, 128, 128, 3, 4, 0, True, False)]


@DTYPES
@pytest.mark.parametrize("case", CASES, ids=lambda c: "k{}s{}-{}to{}-{}x{}-p{}{}{}".format(*c[:7], "-res" * c[7], "-relu" * c[8]))
def test_convbn16_against_fp64(be, case, dtype):
    k, stride, cin, cout, H, W, out_pad, with_res, relu = case
    x, w, scale, shift, res = operands(2, cin, cout, k, stride, H, W, dtype, 1000 + 7 * H + cin + cout + k, with_res)
    check_launch(be, x, w, scale, shift, res, stride, k // 2, dtype, out_pad, relu, f"{case}")


@DTYPES
@pytest.mark.parametrize("H,W", [(9, 13), (32, 37)])
def test_stem_against_conv2d(be, H, W, dtype):
    """the 7 x 7 stride-2 stem through the pack kernel against F.conv2d(stride=2, padding=3): 9 x 13 -> 5 x 7 (every window touches a border), 32 x 37 -> 16 x 19
    (M = 608: five M tiles, a tail)"""
    x, w, scale, shift, _ = operands(2, 3, 64, 7, 2, H, W, dtype, 50 + H, False)
    assert torch.equal(R.conv_bn(x, w, torch.ones(64), torch.zeros(64), 2, 3, relu=False), F.conv2d(x, w, None, stride=2, padding=3))
    check_launch(be, x, w, scale, shift, None, 2, 3, dtype, 0, True, f"stem {H}x{W}", via_pack=True)


def test_stem_one_hot_probes(be):
    """one input element and one weight element are 1: the output is scale where torch's definition puts that tap on that pixel and shift elsewhere (scale = 1,
    shift = 0.25 here) -- a swapped ky / kx or a wrong border cannot pass"""
    H, W, dtype = 9, 13, torch.float16
    for n, ci, py, px, co, ky, kx in ((1, 2, 7, 12, 63, 6, 5), (0, 0, 0, 0, 0, 1, 3), (1, 1, 5, 7, 31, 0, 6)):
        x, w = torch.zeros(2, 3, H, W, dtype=torch.float64), torch.zeros(64, 3, 7, 7, dtype=torch.float64)
        x[n, ci, py, px] = 1.0
        w[co, ci, ky, kx] = 1.0
        want = F.conv2d(x, w, None, stride=2, padding=3) + 0.25
        assert float(want.max()) == 1.25
        got, _, _ = launch(be, x, w, torch.ones(64), torch.full((64,), 0.25), 2, 3, dtype, 0, False)
        assert torch.equal(MR.unframe(got, 0, dtype), want), (n, ci, py, px, co, ky, kx)


def test_convbn16_refusals_and_alignment(be):
    buf = be.dev(np.zeros(1 << 16, np.uint16))
    p = be.ptr(buf)
    good = dict(in_=p, W=p, scale=p, shift=p, residual=None, out=p, N=1, Hi=5, Wi=6, Cin=64, Cout=64, KS=3, stride=1, pad=1, out_pad=0, relu=1, dtype=_abi.DT_F16)
    call = lambda **ch: be.lib.eegclip_convbn16(_abi.ConvBn16Desc(**{**good, **ch}), be.stream)   # noqa: E731
    for change in (dict(KS=5, pad=2), dict(KS=2, pad=1), dict(stride=3), dict(stride=0), dict(pad=0), dict(KS=1, pad=1), dict(Cin=96), dict(Cin=32), dict(Cout=96),
                   dict(Cout=0), dict(Cin=3), dict(KS=7, stride=2, pad=3, Cin=3, Cout=128), dict(KS=7, stride=2, pad=3, Cin=64), dict(KS=7, stride=1, pad=3, Cin=3),
                   dict(KS=11, stride=4, pad=2, Cin=3), dict(out_pad=3), dict(out_pad=-1), dict(relu=2), dict(N=0), dict(Hi=0), dict(dtype=_abi.DT_F32),
                   dict(scale=None), dict(shift=None), dict(in_=None), dict(out=None)):
        assert call(**change) == -1, change
    for change in (dict(in_=p + 8), dict(W=p + 8), dict(out=p + 4), dict(residual=p + 4), dict(scale=p + 2), dict(shift=p + 2)):
        assert call(**change) == -2, change
    assert call(residual=p + 8, scale=p + 4, shift=p + 4, out=p + 8) == 0
    assert be.lib.eegclip_convbn16_in_width(0) == -1 and be.lib.eegclip_convbn16_in_width(1) == 16
    assert be.lib.eegclip_pack_nchw16_stem(p, p, 1, 0, 5, _abi.DT_F16, be.stream) == -1
    assert be.lib.eegclip_pack_nchw16_stem(p, p, 1, 5, 5, _abi.DT_F32, be.stream) == -1
    assert be.lib.eegclip_pack_nchw16_stem(p, p + 4, 1, 5, 5, _abi.DT_F16, be.stream) == -2
    for args in ((1, 0, 8, 64, 0, 0), (1, 8, 8, 60, 0, 0), (1, 8, 8, 64, 3, 0), (1, 8, 8, 64, 0, 3), (0, 8, 8, 64, 0, 0)):
        assert be.lib.eegclip_maxpool16_pad(p, p, *args, _abi.DT_F16, be.stream) == -1, args
    assert be.lib.eegclip_maxpool16_pad(p, p + 4, 1, 8, 8, 64, 0, 0, _abi.DT_F16, be.stream) == -2
    for args in ((0, 2, 2, 64), (1, 0, 2, 64), (1, 2, 2, 60)):
        assert be.lib.eegclip_avgpool16(p, p, *args, _abi.DT_F16, be.stream) == -1, args
    assert be.lib.eegclip_avgpool16(p, p, 1, 2, 2, 64, _abi.DT_F32, be.stream) == -1
    assert be.lib.eegclip_avgpool16(p + 4, p, 1, 2, 2, 64, _abi.DT_F16, be.stream) == -2 and be.lib.eegclip_avgpool16(p, p + 1, 1, 2, 2, 64, _abi.DT_F16, be.stream) == -2
    assert be.lib.eegclip_corr_distance(p, p, 0, 8, p, be.stream) == -1 and be.lib.eegclip_corr_distance(p, p, 1, 1, p, be.stream) == -1
    assert be.lib.eegclip_corr_distance(p, p + 1, 1, 8, p, be.stream) == -2
    be.sync()


@pytest.mark.parametrize("C,in_pad,out_pad", [(64, 0, 0), (64, 1, 1), (72, 0, 2)])
@pytest.mark.parametrize("H,W", [(7, 8), (9, 6), (1, 2)])
def test_maxpool16_pad_negative_input_bit_exact(be, H, W, C, in_pad, out_pad):
    """MaxPool2d(3, 2, 1) with every input negative (a tap read from padding as 0, or a maximum started from 0, would store 0): odd and even sizes, the
    patterns are F.max_pool2d's, the output border stays 0; in_pad = 1 puts zeros around the image that no window may take"""
    for dtype in (torch.float16, torch.bfloat16):
        x = MR.exact(-0.05 - torch.rand(2, C, H, W, generator=torch.Generator().manual_seed(H * W + C)) * 4, dtype)
        ref = F.max_pool2d(x, 3, 2, 1)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        assert tuple(ref.shape) == (2, C, Ho, Wo) and bool((ref < 0).all())
        XIN, OUT = be.dev(MR.frame(x, in_pad, dtype)), be.dev(np.zeros((2, Ho + 2 * out_pad, Wo + 2 * out_pad, C), np.uint16))
        ok(be.lib.eegclip_maxpool16_pad(be.ptr(XIN), be.ptr(OUT), 2, H, W, C, in_pad, out_pad, DT[dtype], be.stream))
        be.sync()
        got = be.host(OUT)
        assert np.array_equal(got, MR.frame(ref, out_pad, dtype))
        assert MR.border_is_zero(got, out_pad)


def test_maxpool16_pad_nan_and_mixed_signs(be):
    """mixed signs against torch bit for bit; a NaN tap wins, as in torch"""
    dtype = torch.float16
    x = MR.exact(torch.randn(1, 64, 6, 7, generator=torch.Generator().manual_seed(3)), dtype)
    x[0, 5, 3, 3] = float("nan")
    ref = F.max_pool2d(x, 3, 2, 1)
    XIN, OUT = be.dev(MR.frame(x, 0, dtype)), be.dev(np.zeros((1, 3, 4, 64), np.uint16))
    ok(be.lib.eegclip_maxpool16_pad(be.ptr(XIN), be.ptr(OUT), 1, 6, 7, 64, 0, 0, DT[dtype], be.stream))
    be.sync()
    got = MR.unframe(be.host(OUT), 0, dtype)
    assert int(ref.isnan().sum()) == 4 and torch.equal(got.isnan(), ref.isnan()) and torch.equal(got.nan_to_num(7.0), ref.nan_to_num(7.0))


@DTYPES
@pytest.mark.parametrize("N,H,W,C", [(3, 2, 2, 64), (2, 7, 7, 2048), (1, 5, 3, 72), (40, 1, 1, 64)])
def test_avgpool16_against_fp64(be, N, H, W, C, dtype):
    """post-ReLU-like (non-negative) values: within (H W + 1) 2^-24 relative of the fp64 mean of the same 16-bit values; mixed signs: the same count of roundings
    relative to the mean of the absolute values.  (40, 1, 1, 64) is more than one workgroup of 256 threads."""
    g = torch.Generator().manual_seed(N + H + C)
    for signed in (False, True):
        x = MR.exact(torch.randn(N, C, H, W, generator=g) if signed else torch.rand(N, C, H, W, generator=g) * 3, dtype)
        XIN, OUT = be.dev(MR.frame(x, 0, dtype)), be.zeros((N, C), np.float32)
        ok(be.lib.eegclip_avgpool16(be.ptr(XIN), be.ptr(OUT), N, H, W, C, DT[dtype], be.stream))
        be.sync()
        got = torch.from_numpy(be.host(OUT)).double()
        ref, scale = x.mean((2, 3)), x.abs().mean((2, 3))
        err = (got - ref).abs()
        print(f"\n[resnet] avgpool {N}x{H}x{W}x{C} {dtype} signed={signed}: max err / bound {float((err / ((H * W + 1) * 2.0 ** -24 * scale)).max()):.3f}", end=" ")
        assert bool((err <= (H * W + 1) * 2.0 ** -24 * scale).all())
        if not signed:
            assert torch.equal(scale, ref)


CORR_BOUND = 64 * 2.0 ** -24


@pytest.mark.parametrize("D", [2, 63, 2048])
@pytest.mark.parametrize("N", [1, 5])
def test_corr_distance_against_scipy(be, N, D):
    """rows with a large common offset (mean 100 x the spread, each row its own) and plain rows, correlated at 0.6: within 64 x 2^-24 absolute of scipy in fp64
    on the same fp32 values"""
    rng = np.random.default_rng(10 * N + D)
    worst = 0.0
    for offset in (0.0, 100.0):
        a = rng.standard_normal((N, D))
        b = 0.6 * a + 0.8 * rng.standard_normal((N, D))
        a, b = (a + offset * (1 + np.arange(N))[:, None]).astype(np.float32), (b - 0.5 * offset).astype(np.float32)
        A, B, OUT = be.dev(a), be.dev(b), be.zeros((N,), np.float32)
        ok(be.lib.eegclip_corr_distance(be.ptr(A), be.ptr(B), N, D, be.ptr(OUT), be.stream))
        be.sync()
        got, ref = be.host(OUT).astype(np.float64), R.correlation(a, b)
        worst = max(worst, float(np.abs(got - ref).max()))
        assert (np.abs(got - ref) <= CORR_BOUND).all(), (offset, got, ref)
        if D > 2:
            assert 0.05 < ref.min() and ref.max() < 1.95
    print(f"\n[resnet] corr_distance N={N} D={D}: max |d - scipy| {worst:.2e} = {worst * 2 ** 24:.1f} x 2^-24", end=" ")


def test_corr_distance_constant_row_is_nan(be):
    a = np.stack([np.full(63, 2.5, np.float32), np.arange(63, dtype=np.float32)])
    b = np.stack([np.arange(63, dtype=np.float32), np.arange(63, dtype=np.float32)[::-1].copy()])
    A, B, OUT = be.dev(a), be.dev(b), be.zeros((2,), np.float32)
    ok(be.lib.eegclip_corr_distance(be.ptr(A), be.ptr(B), 2, 63, be.ptr(OUT), be.stream))
    be.sync()
    got = be.host(OUT)
    assert np.isnan(got[0]) and abs(float(got[1]) - 2.0) <= CORR_BOUND          # (the second pair is anti-correlated: r = -1)
