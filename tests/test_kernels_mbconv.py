"""The EffNet-B row's entry points through the C ABI on both backends (CPU lane emulator / MI355X): csrc/mbconv.hip's eegclip_dwconv16 (with its pooled
slabs), eegclip_se_gate16 and eegclip_gate_mul16, and csrc/metric_nets.hip's eegclip_convbnact16 / eegclip_pack_nchw16_pad1, against tests/effnet_ref.py (fp64
torch.nn.functional on the CPU).  Operands (inputs, weights, residuals) are values exact in the 16-bit dtype, scale, shift and the slabs are fp32, and the
references are fp64 of those same values.  u = 2^-11 (fp16) / 2^-8 (bf16) is the one rounding at a store, tiny = 2^-25 in fp16 (half the spacing of its
subnormals), 0 in bf16.

Depthwise (per element).  The kernel forms v = scale acc + shift from k^2 products accumulated in fp32 and stores round(silu(v)):
    |v - v_ref| <= A = (k^2 + 4) 2^-23 (|scale| (|x| (*) |w|) + |shift|)
(k^2 terms and four more fp32 roundings, as in tests/test_kernels_resnet.py); SiLU's slope is at most 1.1 (its derivative peaks at 1.0998 near x = 2.4), so
    |y - silu(v_ref)| <= u |silu(v_ref)| + tiny + 1.1 A (1 + u).
SiLU's own fp32 evaluation (one exponential, one sum, one quotient: a few 2^-24 relative to |silu| <= |v| <= A 2^23 / (k^2 + 4)) sits inside the generous count of
A: k^2 + 4 roundings of 2^-23 where the sums pay at most 2^-24 each.

Pooled slabs.  The consumer's fixed-order sum over S is compared with the fp64 sum of the kernel's OWN stored outputs: Ho Wo fp32 additions of exact
16-bit values, |sum - ref| <= Ho Wo 2^-24 sum |y|.

Gate.  mean = (sum_s slab) / HW, h = silu(W1 mean + b1), g = sigmoid(W2 h + b2) with fp32 sums of C and sq terms.  With r = (C + sq + 8) 2^-23:
    |h - h_ref| <= 1.1 r (|W1| |mean| + |b1|) =: dh          (|mean| from sum |slab|, which also covers the S additions and the division)
    |g - g_ref| <= 1/4 (|W2| dh + r (|W2| |h_ref| + |b2|)) + 2^-22      (sigmoid's slope is at most 1/4; 2^-22: its own fp32 evaluation, g <= 1)

Multiply: bit-equal to (y.float() * gate).to(dtype).

Convolution + activation: tests/test_kernels_resnet.py's bound with the activation's slope,
    |y - ref| <= u |ref| + tiny + 1.1 (K + 4) 2^-23 (|scale| (|x| (*) |w|) + |shift|) + 2^-22 |residual|,     K = KS^2 Cin
(the residual is exact and enters by one fp32 addition; 2^-22 of it covers that addition's rounding of the sum)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import effnet_ref as R
import metric_nets_ref as MR
from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi

DT = {torch.float16: _abi.DT_F16, torch.bfloat16: _abi.DT_BF16}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
EINVAL, EALIGN = -1, -2


def out_size(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


# ------------------------------------------------------------------------------------------------------------------------------------------ depthwise
def run_dw(be, x, w, scale, shift, stride, dtype):
    """one eegclip_dwconv16 launch on x (N, C, H, W), w (C, 1, k, k) -> (stored values (N, C, Ho, Wo) fp64, slabs (N, S, C) fp32 numpy)"""
    N, C, H, W = x.shape
    k = w.shape[2]
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    S = be.lib.eegclip_dwconv16_slabs(H, W, k, stride)
    assert S == -(-(Ho * -(-Wo // 4)) // 32)
    XIN, WP = be.dev(MR.frame(x, k // 2, dtype)), be.dev(R.dw_weight(w, dtype))
    SC, SH = be.dev(scale.float().numpy()), be.dev(shift.float().numpy())
    OUT = be.dev(np.full((N, Ho, Wo, C), 0x7e00 if dtype == torch.float16 else 0x7fc0, np.uint16))         # NaN patterns: every element must be written
    SLAB = be.dev(np.full((N, S, C), np.nan, np.float32))
    ok(be.lib.eegclip_dwconv16(be.ptr(XIN), be.ptr(WP), be.ptr(SC), be.ptr(SH), be.ptr(OUT), be.ptr(SLAB), N, H, W, C, k, stride, DT[dtype], be.stream))
    be.sync()
    return MR.unframe(be.host(OUT), 0, dtype), be.host(SLAB)


def dw_operands(N, C, k, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = MR.exact(torch.randn(N, C, H, W, generator=g) * 1.5, dtype)
    w = MR.exact(torch.randn(C, 1, k, k, generator=g) / k, dtype)
    scale = ((0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)).float()      # both signs
    shift = (0.5 * torch.randn(C, generator=g)).float()
    return x, w, scale, shift


# (k, stride) x sizes: 9 x 11 and 8 x 10 (odd and even: which bottom / right taps are read), 3 x 4 and 1 x 1 (smaller than the kernel); widths 11, 10, 6, 5, 2, 1
# are no multiples of the thread's run of 4 pixels.  C = 192: three channel blocks.  9 x 11 at stride 1 is 9 x 3 = 27 runs (one slab, partly filled);
# the 21 x 30 case is 21 x 8 = 168 runs: S = 6, the last slab ragged (8 runs of 32).
DW_CASES = [(k, s, H, W, C) for k in (3, 5) for s in (1, 2) for (H, W, C) in ((9, 11, 64), (8, 10, 192), (3, 4, 64), (1, 1, 64))] + [(3, 1, 21, 30, 72), (5, 2, 41, 59, 64)]


@DTYPES
@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "k{}s{}-{}x{}-c{}".format(*c))
def test_dwconv16_against_fp64_and_pooled_slabs(be, case, dtype):
    k, stride, H, W, C = case
    N = 2
    x, w, scale, shift = dw_operands(N, C, k, H, W, dtype, 100 * k + 10 * stride + H + C)
    y, slab = run_dw(be, x, w, scale, shift, stride, dtype)
    pre = R.dw_pre(x, w, scale, shift, stride)
    ref = R.silu(pre)
    Ho, Wo = out_size(H, k, stride), out_size(W, k, stride)
    assert tuple(ref.shape) == tuple(y.shape) == (N, C, Ho, Wo)
    A = (k * k + 4) * 2.0 ** -23 * (scale.double().abs()[None, :, None, None] * R.dw_abs(x, w, stride) + shift.double().abs()[None, :, None, None])
    u = R.UNIT[dtype]
    bound = u * ref.abs() + TINY[dtype] + 1.1 * A * (1 + u)
    err = (y - ref).abs()
    print(f"\n[mbconv] dw {case} {dtype}: max err {float(err.max()):.2e}, max err / bound {float((err / bound).max()):.3f}", end=" ")
    assert not bool(y.isnan().any()) and bool((err <= bound).all())
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    if H * W > 1:
        assert float((pre < 0).double().mean()) > 0.2 and float((pre > 0).double().mean()) > 0.2
    # the pooled sums: the consumer's order (increasing s, fp32) against the fp64 sum of the kernel's own stored outputs
    S = slab.shape[1]
    assert slab.shape == (N, S, C) and not np.isnan(slab).any()
    total = np.zeros((N, C), np.float32)
    for s in range(S):
        total = total + slab[:, s]
    want, mag = y.sum((2, 3)), y.abs().sum((2, 3))
    perr = (torch.from_numpy(total).double() - want).abs()
    pbound = Ho * Wo * 2.0 ** -24 * mag
    print(f"S={S} pooled max err / bound {float((perr / pbound.clamp_min(1e-300)).max()):.3f}", end=" ")
    assert bool((perr <= pbound).all())
    if case == (3, 1, 21, 30, 72):
        assert S == 6 and (21 * 8) % 32 != 0
    if case == (5, 2, 41, 59, 64):
        assert S == 6 and Wo % 4 != 0 and (Ho * 8) % 32 != 0


def test_dwconv16_one_hot_probes(be):
    """one input element and one weight element are 1, scale = 1, shift = 0: the output is silu(1) exactly where torch's definition puts that tap and 0
    elsewhere -- a swapped ky / kx, a channel shift or a wrong border cannot pass"""
    dtype = torch.float16
    one = float(torch.tensor(1.0, dtype=torch.float64).mul(torch.sigmoid(torch.tensor(1.0, dtype=torch.float64))).to(dtype))
    for k, stride, H, W, (n, c, py, px, ky, kx) in ((3, 1, 9, 11, (1, 63, 8, 10, 2, 1)), (3, 1, 9, 11, (0, 9, 0, 3, 0, 2)), (3, 2, 9, 11, (0, 0, 0, 0, 1, 1)),
                                                    (3, 2, 8, 10, (1, 17, 6, 9, 1, 2)), (5, 1, 9, 11, (0, 8, 4, 5, 4, 1)), (5, 1, 9, 11, (1, 7, 0, 10, 1, 3)),
                                                    (5, 2, 9, 11, (1, 40, 8, 2, 2, 4)), (5, 2, 8, 10, (0, 33, 3, 9, 3, 3)), (5, 1, 3, 4, (1, 5, 2, 3, 3, 2))):
        x, w = torch.zeros(2, 64, H, W, dtype=torch.float64), torch.zeros(64, 1, k, k, dtype=torch.float64)
        x[n, c, py, px] = 1.0
        w[c, 0, ky, kx] = 1.0
        hit = F.conv2d(x, w, None, stride=stride, padding=k // 2, groups=64)
        assert float(hit.sum()) == 1.0, "the probe must land on an output pixel"
        y, slab = run_dw(be, x, w, torch.ones(64), torch.zeros(64), stride, dtype)
        assert torch.equal(y, hit * one), (k, stride, H, W, n, c, py, px, ky, kx)
        assert float(slab.sum()) == one and float(slab[n, :, c].sum()) == one


# ------------------------------------------------------------------------------------------------------------------------------------------ gate
@DTYPES
@pytest.mark.parametrize("C,sq,S,HW", [(64, 1, 1, 1), (64, 6, 3, 77), (704, 28, 2, 64), (1920, 80, 1, 9), (704, 6, 5, 4096), (64, 80, 2, 30)])
def test_se_gate16_against_fp64(be, C, sq, S, HW, dtype):
    N = 3
    g = torch.Generator().manual_seed(C + sq + S)
    slab = (torch.randn(N, S, C, generator=g) * (HW / S)).float()                       # pooled sums of values of order 1
    w1 = MR.exact(torch.randn(sq, C, generator=g) / C ** 0.5, dtype)
    b1 = MR.exact(0.5 * torch.randn(sq, generator=g), dtype)
    w2 = MR.exact(2 * torch.randn(C, sq, generator=g) / sq ** 0.5, dtype)
    b2 = MR.exact(torch.randn(C, generator=g), dtype)
    P, W1, B1, W2, B2 = be.dev(slab.numpy()), be.dev(MR.bits(w1, dtype)), be.dev(MR.bits(b1, dtype)), be.dev(MR.bits(w2, dtype)), be.dev(MR.bits(b2, dtype))
    G = be.dev(np.full((N, C), np.nan, np.float32))
    ok(be.lib.eegclip_se_gate16(be.ptr(P), be.ptr(W1), be.ptr(B1), be.ptr(W2), be.ptr(B2), be.ptr(G), N, S, HW, C, sq, DT[dtype], be.stream))
    be.sync()
    got = torch.from_numpy(be.host(G)).double()
    mean, amean = slab.double().sum(1) / HW, slab.double().abs().sum(1) / HW
    h = R.silu(mean @ w1.t() + b1)
    ref = torch.sigmoid(h @ w2.t() + b2)
    r = (C + sq + 8) * 2.0 ** -23
    dh = 1.1 * r * (amean @ w1.abs().t() + b1.abs())
    bound = 0.25 * (dh @ w2.abs().t() + r * (h.abs() @ w2.abs().t() + b2.abs())) + 2.0 ** -22
    err = (got - ref).abs()
    print(f"\n[mbconv] gate C={C} sq={sq} S={S} {dtype}: max err {float(err.max()):.2e}, max err / bound {float((err / bound).max()):.3f}", end=" ")
    assert bool((err <= bound).all())
    assert float(ref.min()) < 0.3 and float(ref.max()) > 0.7                            # both ends of the sigmoid are exercised


@DTYPES
@pytest.mark.parametrize("N,HW,C", [(2, 1, 64), (3, 35, 72), (2, 300, 192)])
def test_gate_mul16_bit_equal(be, N, HW, C, dtype):
    g = torch.Generator().manual_seed(HW + C)
    y = (torch.randn(N, HW, C, generator=g) * 3).to(dtype)
    gate = torch.rand(N, C, generator=g).float()
    Y, G = be.dev(MR.bits(y, dtype)), be.dev(gate.numpy())
    ok(be.lib.eegclip_gate_mul16(be.ptr(Y), be.ptr(G), N, HW, C, DT[dtype], be.stream))
    be.sync()
    want = (y.float() * gate[:, None, :]).to(dtype)
    got, bits = be.host(Y), MR.bits(want, dtype)
    bad = np.argwhere(got != bits)
    print(f"\n[mbconv] gate_mul {N}x{HW}x{C} {dtype}: {len(bad)} of {got.size} patterns differ", *(f"y={float(y[tuple(i)])!r} gate={float(gate[i[0], i[2]])!r} got={int(got[tuple(i)]):#06x} "
                                                                                                  f"want={int(bits[tuple(i)]):#06x}" for i in bad[:4]), end=" ")
    assert np.array_equal(got, bits)


# ------------------------------------------------------------------------------------------------------------------------------------------ convolution + activation
def run_conv(be, x, w, scale, shift, stride, pad, dtype, in_pad, out_pad, act, residual=None, via_pack=False):
    """one eegclip_convbnact16 launch on x (N, Cin, H, W) -> (output frame patterns, Ho, Wo)"""
    N, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if cin == 3:
        width = be.lib.eegclip_convbnact16_in_width(W)
        assert width % 2 == 0 and width >= max(W + 2, 2 * (Wo - 1) + 16)
        host = R.stem_frame(x, width, dtype)
        if via_pack:
            XIN, PLANES = be.dev(np.zeros_like(host)), be.dev(MR.bits(x, dtype))
            ok(be.lib.eegclip_pack_nchw16_pad1(be.ptr(PLANES), be.ptr(XIN), N, H, W, DT[dtype], be.stream))
            be.sync()
            assert np.array_equal(be.host(XIN), host)
        else:
            XIN = be.dev(host)
    else:
        f = MR.frame(x, in_pad, dtype)
        if in_pad:                                            # a 1 x 1 layer must skip the border: fill it with a value that would show
            inner = f[:, in_pad:-in_pad, in_pad:-in_pad].copy()
            f[:] = MR.bits(torch.tensor(100.0), dtype)
            f[:, in_pad:-in_pad, in_pad:-in_pad] = inner
        XIN = be.dev(f)
    WP = be.dev(MR.pack_weight(w, dtype))
    SC, SH = be.dev(scale.float().numpy()), be.dev(shift.float().numpy())
    RES = be.dev(MR.frame(residual, out_pad, dtype)) if residual is not None else None
    OUT = be.dev(np.zeros((N, Ho + 2 * out_pad, Wo + 2 * out_pad, cout), np.uint16))
    d = _abi.ConvBnAct16Desc(in_=be.ptr(XIN), W=be.ptr(WP), scale=be.ptr(SC), shift=be.ptr(SH), residual=be.ptr(RES), out=be.ptr(OUT), N=N, Hi=H, Wi=W, Cin=cin,
                             Cout=cout, KS=k, stride=stride, pad=pad, in_pad=in_pad, out_pad=out_pad, act=act, dtype=DT[dtype])
    ok(be.lib.eegclip_convbnact16(d, be.stream))
    be.sync()
    return be.host(OUT), Ho, Wo


def conv_operands(N, cin, cout, k, H, W, Ho, Wo, dtype, seed, with_res):
    g = torch.Generator().manual_seed(seed)
    x = MR.exact(torch.randn(N, cin, H, W, generator=g), dtype)
    w = MR.exact(1.5 * torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, dtype)
    scale = ((0.5 + torch.rand(cout, generator=g)) * torch.where(torch.rand(cout, generator=g) < 0.5, -1.0, 1.0)).float()
    shift = (0.5 * torch.randn(cout, generator=g)).float()
    res = MR.exact(torch.randn(N, cout, Ho, Wo, generator=g), dtype) if with_res else None
    return x, w, scale, shift, res


def check_conv(be, x, w, scale, shift, res, stride, pad, dtype, in_pad, out_pad, act, label, via_pack=False):
    cout, cin, k, _ = w.shape
    got, Ho, Wo = run_conv(be, x, w, scale, shift, stride, pad, dtype, in_pad, out_pad, act, res, via_pack)
    ref, pre = R.conv_bn_act(x, w, scale, shift, stride, pad, act, res)
    assert tuple(ref.shape) == (x.shape[0], cout, Ho, Wo)
    y = MR.unframe(got, out_pad, dtype)
    mag = scale.double().abs()[None, :, None, None] * MR.conv_abs(x, w, stride, pad) + shift.double().abs()[None, :, None, None]
    bound = R.UNIT[dtype] * ref.abs() + TINY[dtype] + 1.1 * (cin * k * k + 4) * 2.0 ** -23 * mag
    if res is not None:
        bound = bound + 2.0 ** -22 * res.double().abs()
    err = (y - ref).abs()
    print(f"\n[mbconv] conv {label} {dtype}: max err {float(err.max()):.2e}, max err / bound {float((err / bound).max()):.3f}", end=" ")
    assert bool((err <= bound).all())
    assert MR.border_is_zero(got, out_pad)
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    assert float((pre < 0).double().mean()) > 0.2 and float((pre > 0).double().mean()) > 0.2
    if act != 1:
        assert float((ref < 0).double().mean()) > 0.2         # SiLU and the identity keep negative values: a ReLU in their place cannot pass


# (Cin, Cout, H, W, in_pad, out_pad, act, residual), N = 2: 9 x 11 is M = 198 (two M tiles, the second a tail)
CONV_CASES = [(64, 64, 9, 11, 0, 0, 2, False), (64, 128, 9, 11, 0, 1, 2, False), (128, 192, 8, 10, 1, 2, 2, False), (192, 64, 9, 11, 0, 0, 0, True),
              (192, 128, 3, 4, 0, 0, 0, False), (64, 64, 9, 11, 1, 1, 0, True), (128, 64, 1, 1, 2, 0, 1, False), (64, 192, 5, 7, 0, 0, 2, True)]


@DTYPES
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "{}to{}-{}x{}-ip{}-op{}-act{}{}".format(*c[:7], "-res" * c[7]))
def test_convbnact16_pointwise_against_fp64(be, case, dtype):
    cin, cout, H, W, in_pad, out_pad, act, with_res = case
    x, w, scale, shift, res = conv_operands(2, cin, cout, 1, H, W, H, W, dtype, 7 * H + cin + cout + act, with_res)
    check_conv(be, x, w, scale, shift, res, 1, 0, dtype, in_pad, out_pad, act, f"{case}")


@DTYPES
@pytest.mark.parametrize("H,W", [(9, 13), (32, 37)])
def test_stem_against_conv2d(be, H, W, dtype):
    """the 3 x 3 stride-2 stem through the pack kernel against F.conv2d(stride=2, padding=1): 9 x 13 -> 5 x 7, 32 x 37 -> 16 x 19 (M = 608: five M tiles, a
    tail).  The kernel's tile has 64 filters; EfficientNet's stem has 32: with the packed rows 32 .. 63, their scale and their shift zero, those output channels
    are exactly 0 and the others are unchanged"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, w, scale, shift, _ = conv_operands(2, 3, 64, 3, H, W, Ho, Wo, dtype, 50 + H, False)
    ref, _ = R.conv_bn_act(x, w, torch.ones(64), torch.zeros(64), 2, 1, 0)
    assert torch.equal(ref, F.conv2d(x, w, None, stride=2, padding=1)) and tuple(ref.shape) == (2, 64, Ho, Wo)
    check_conv(be, x, w, scale, shift, None, 2, 1, dtype, 0, 1, 2, f"stem {H}x{W}", via_pack=True)
    full, _, _ = run_conv(be, x, w, scale, shift, 2, 1, dtype, 0, 1, 2)
    w[32:], scale[32:], shift[32:] = 0.0, 0.0, 0.0
    half, _, _ = run_conv(be, x, w, scale, shift, 2, 1, dtype, 0, 1, 2)
    assert not half[..., 32:].any() and np.array_equal(half[..., :32], full[..., :32]) and full[..., 32:].any()


def test_convbnact16_one_hot_probes(be):
    """one input element and one weight element are 1, scale = 1, shift = 0.25, no activation: the output is 1.25 where torch's definition puts that tap and 0.25
    elsewhere, for the stem (a swapped ky / kx or a wrong border cannot pass) and for a 1 x 1 layer (a channel shift cannot pass)"""
    dtype = torch.float16
    for n, ci, py, px, co, ky, kx in ((1, 2, 7, 12, 63, 2, 1), (0, 0, 0, 0, 0, 1, 1), (1, 1, 5, 7, 17, 0, 2), (0, 2, 4, 11, 5, 1, 0)):
        x, w = torch.zeros(2, 3, 9, 13, dtype=torch.float64), torch.zeros(64, 3, 3, 3, dtype=torch.float64)
        x[n, ci, py, px] = 1.0
        w[co, ci, ky, kx] = 1.0
        want = F.conv2d(x, w, None, stride=2, padding=1) + 0.25
        assert float(want.max()) == 1.25
        got, _, _ = run_conv(be, x, w, torch.ones(64), torch.full((64,), 0.25), 2, 1, dtype, 0, 0, 0)
        assert torch.equal(MR.unframe(got, 0, dtype), want), (n, ci, py, px, co, ky, kx)
    for n, ci, py, px, co in ((1, 127, 4, 6, 64), (0, 0, 0, 0, 191), (1, 65, 2, 0, 0)):
        x, w = torch.zeros(2, 128, 5, 7, dtype=torch.float64), torch.zeros(192, 128, 1, 1, dtype=torch.float64)
        x[n, ci, py, px] = 1.0
        w[co, ci, 0, 0] = 1.0
        want = F.conv2d(x, w) + 0.25
        assert float(want.sum()) == 0.25 * want.numel() + 1.0
        got, _, _ = run_conv(be, x, w, torch.ones(192), torch.full((192,), 0.25), 1, 0, dtype, 0, 0, 0)
        assert torch.equal(MR.unframe(got, 0, dtype), want), (n, ci, py, px, co)


# ------------------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_alignment(be):
    buf = be.dev(np.zeros(1 << 16, np.uint16))
    p = be.ptr(buf)
    L, f16 = be.lib, _abi.DT_F16
    good = dict(in_=p, W=p, scale=p, shift=p, residual=None, out=p, N=1, Hi=5, Wi=6, Cin=64, Cout=64, KS=1, stride=1, pad=0, in_pad=0, out_pad=0, act=2, dtype=f16)
    stem = dict(KS=3, stride=2, pad=1, Cin=3, Cout=64)
    call = lambda **ch: L.eegclip_convbnact16(_abi.ConvBnAct16Desc(**{**good, **ch}), be.stream)   # noqa: E731
    for change in (dict(KS=3, pad=1), dict(KS=5, pad=2), dict(stride=2), dict(stride=0), dict(pad=1), dict(Cin=96), dict(Cin=32), dict(Cout=96), dict(Cout=0),
                   dict(Cin=3), dict(stem, Cout=32), dict(stem, Cout=128), dict(stem, stride=1), dict(stem, pad=0), dict(stem, in_pad=1), dict(stem, Cin=64),
                   dict(KS=7, stride=2, pad=3, Cin=3), dict(in_pad=3), dict(in_pad=-1), dict(out_pad=3), dict(out_pad=-1), dict(act=3), dict(act=-1), dict(N=0),
                   dict(Hi=0), dict(Wi=0), dict(dtype=_abi.DT_F32), dict(scale=None), dict(shift=None), dict(in_=None), dict(W=None), dict(out=None)):
        assert call(**change) == EINVAL, change
    for change in (dict(in_=p + 8), dict(W=p + 8), dict(out=p + 4), dict(residual=p + 4), dict(scale=p + 2), dict(shift=p + 2)):
        assert call(**change) == EALIGN, change
    assert call(residual=p + 8, scale=p + 4, shift=p + 4, out=p + 8) == 0 and call(**stem) == 0 and call(in_pad=2, act=0) == 0
    assert L.eegclip_convbnact16_in_width(0) == EINVAL and L.eegclip_convbnact16_in_width(1) == 16 and L.eegclip_convbnact16_in_width(37) == 52
    assert L.eegclip_pack_nchw16_pad1(p, p, 1, 0, 5, f16, be.stream) == EINVAL and L.eegclip_pack_nchw16_pad1(p, p, 1, 5, 5, _abi.DT_F32, be.stream) == EINVAL
    assert L.eegclip_pack_nchw16_pad1(None, p, 1, 5, 5, f16, be.stream) == EINVAL and L.eegclip_pack_nchw16_pad1(p, p + 4, 1, 5, 5, f16, be.stream) == EALIGN
    # depthwise: (N, H, W, C, k, stride, dtype)
    dw = lambda a=p, w=p, sc=p, sh=p, o=p, pl=p, args=(1, 5, 6, 64, 3, 1, f16): L.eegclip_dwconv16(a, w, sc, sh, o, pl, *args, be.stream)   # noqa: E731
    for args in ((1, 5, 6, 64, 4, 1, f16), (1, 5, 6, 64, 7, 1, f16), (1, 5, 6, 64, 1, 1, f16), (1, 5, 6, 64, 3, 3, f16), (1, 5, 6, 64, 3, 0, f16), (1, 5, 6, 60, 3, 1, f16),
                 (1, 5, 6, 0, 3, 1, f16), (1, 5, 6, 4, 3, 1, f16), (0, 5, 6, 64, 3, 1, f16), (65536, 5, 6, 64, 3, 1, f16), (1, 0, 6, 64, 3, 1, f16), (1, 5, 0, 64, 3, 1, f16),
                 (1, 5, 6, 64, 3, 1, _abi.DT_F32)):
        assert dw(args=args) == EINVAL, args
    for kw in (dict(a=None), dict(w=None), dict(sc=None), dict(sh=None), dict(o=None), dict(pl=None)):
        assert dw(**kw) == EINVAL, kw
    for kw in (dict(a=p + 8), dict(w=p + 8), dict(sc=p + 4), dict(sh=p + 8), dict(o=p + 2), dict(pl=p + 2)):
        assert dw(**kw) == EALIGN, kw
    assert dw(pl=p + 4, args=(1, 5, 6, 72, 5, 2, f16)) == 0
    for args in ((0, 6, 3, 1), (5, 0, 3, 1), (5, 6, 4, 1), (5, 6, 3, 3)):
        assert L.eegclip_dwconv16_slabs(*args) == EINVAL, args
    assert L.eegclip_dwconv16_slabs(1, 1, 5, 2) == 1 and L.eegclip_dwconv16_slabs(128, 128, 3, 1) == 128 and L.eegclip_dwconv16_slabs(255, 255, 3, 2) == 128
    # gate: (N, S, HW, C, sq, dtype)
    gt = lambda pl=p, w1=p, b1=p, w2=p, b2=p, g=p, args=(1, 2, 30, 64, 6, f16): L.eegclip_se_gate16(pl, w1, b1, w2, b2, g, *args, be.stream)   # noqa: E731
    for args in ((0, 2, 30, 64, 6, f16), (1, 0, 30, 64, 6, f16), (1, 2, 0, 64, 6, f16), (1, 2, 30, 0, 6, f16), (1, 2, 30, 8200, 6, f16), (1, 2, 30, 64, 0, f16),
                 (1, 2, 30, 64, 4097, f16), (1, 2, 30, 64, 6, _abi.DT_F32)):
        assert gt(args=args) == EINVAL, args
    for kw in (dict(pl=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(g=None)):
        assert gt(**kw) == EINVAL, kw
    for kw in (dict(pl=p + 2), dict(g=p + 2), dict(w1=p + 1), dict(b1=p + 1), dict(w2=p + 1), dict(b2=p + 1)):
        assert gt(**kw) == EALIGN, kw
    assert gt(pl=p + 4, g=p + 4, w1=p + 2, b1=p + 2, w2=p + 2, b2=p + 2) == 0
    # multiply: (N, HW, C, dtype)
    for args in ((0, 4, 64, f16), (1, 0, 64, f16), (1, 4, 60, f16), (1, 4, 0, f16), (1, 4, 64, _abi.DT_F32)):
        assert L.eegclip_gate_mul16(p, p, *args, be.stream) == EINVAL, args
    assert L.eegclip_gate_mul16(None, p, 1, 4, 64, f16, be.stream) == EINVAL and L.eegclip_gate_mul16(p, None, 1, 4, 64, f16, be.stream) == EINVAL
    assert L.eegclip_gate_mul16(p + 8, p, 1, 4, 64, f16, be.stream) == EALIGN and L.eegclip_gate_mul16(p, p + 4, 1, 4, 64, f16, be.stream) == EALIGN
    assert L.eegclip_gate_mul16(p, p, 1, 4, 64, f16, be.stream) == 0
    be.sync()
