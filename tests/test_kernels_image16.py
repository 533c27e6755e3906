"""The 16-bit image kernels (csrc/vae.hip, csrc/unet.hip) through the C ABI on both backends, in fp16 AND bf16, against numpy fp64 with PER-ELEMENT bounds
derived from the number formats (a correctly rounded store plus the fp32 arithmetic in front of it), at the smallest shapes that reach a second M tile /
pixel block / loop trip: conv16 (matrix forms, direct form, an exact one-hot test of the address maps), groupnorm16 (output, `sums`, large |mean| / sd),
softmax_rows16, vae_sample16, geglu16, concat16.  tests/test_kernels_vae.py and test_kernels_unet.py keep the bf16-only, global-tolerance versions."""
import math

import numpy as np
import pytest

from backends import be, ok  # noqa: F401
from eeg_image_decode_amd import _abi
from test_kernels_gemm16 import DT, from16, to16
from test_kernels_vae import conv_ref, frame

DTS = ["f16", "bf16"]
SENTINEL = 0x7FC0                                                            # a NaN in both formats


def q16(x, dt):
    """round to the dtype: (bit pattern, value as fp64)"""
    bits, v = to16(np.ascontiguousarray(x, np.float32), dt)
    return bits, v.astype(np.float64)


def frame16(x, dt, pad, border=0):
    """(N, C, H, W), representable in dt -> padded NHWC uint16; the one-pixel border holds `border`"""
    x = np.asarray(x, np.float32)
    if dt == "bf16":
        f = frame(x, pad)
    else:
        N, C, H, W = x.shape
        f = np.zeros((N, H + 2 * pad, W + 2 * pad, C), np.uint16)
        f[:, pad:pad + H, pad:pad + W, :] = to16(np.ascontiguousarray(x.transpose(0, 2, 3, 1)), dt)[0]
    if pad and border:
        f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = border, border, border, border
    return f


def unframe16(f, dt, pad):
    """padded NHWC uint16 -> (N, C, H, W) fp64 of the interior"""
    inner = f[:, pad:f.shape[1] - pad, pad:f.shape[2] - pad, :]
    return from16(inner, dt).astype(np.float64).transpose(0, 3, 1, 2)


def border_is(f, pad, value):
    return not pad or bool((f[:, 0] == value).all() and (f[:, -1] == value).all() and (f[:, :, 0] == value).all() and (f[:, :, -1] == value).all())


def ulp16(ref, dt):
    """spacing of the dtype at |ref|: fp16 np.spacing(|ref| as float16); bf16 2 ** (floor(log2 |ref|) - 7) (the smallest normal's below it)"""
    a = np.abs(np.asarray(ref, np.float64))
    if dt == "f16":
        return np.spacing(a.astype(np.float16)).astype(np.float64)
    e = np.frexp(a)[1] - 1                                                   # floor(log2 a); 0 for a == 0
    return np.ldexp(1.0, np.maximum(np.where(a == 0, -126, e), -126) - 7)


def report(name, ratio):
    """every figure is printed before it is asserted (pytest -s shows them)"""
    print(f"{name}: max err / bound = {ratio:.3f}")
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------------- conv16

def conv_geometry(KS, stride, up, pads):
    """-> (pads of conv_ref (top, left, bottom, right), (pad_top, pad_left) of the descriptor)"""
    if up:
        return (1, 1, 1, 1), (1, 1)
    if stride == 2:                                                          # pads (1, 1): the UNet's Downsample2D; (0, 0): the VAE's, which pads bottom / right only
        return (pads[0], pads[1], 1, 1), pads
    p = (KS - 1) // 2
    return (p, p, p, p), (p, p)


def run_conv16(be, dt, x, w, b, res, cb, KS, stride, up, pads, in_pad, out_pad):
    """x (N, Cin, H, W), w (Cout, Cin, KS, KS), b (Cout) / res (N, Cout, Ho, Wo) / cb (N, Cout) or None, all representable in dt -> ((N, Cout, Ho, Wo) fp64, ref pads).
    Output and residual frames carry a NaN border that must survive; 128 NaN rows follow the weights"""
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    rpads, dpads = conv_geometry(KS, stride, up, pads)
    Hs, Ws = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hs + rpads[0] + rpads[2] - KS) // stride + 1, (Ws + rpads[1] + rpads[3] - KS) // stride + 1
    wp = np.full((Cout + 128, KS * KS, Cin), SENTINEL, np.uint16)
    wp[:Cout] = to16(np.ascontiguousarray(w.transpose(0, 2, 3, 1), np.float32).reshape(Cout, KS * KS, Cin), dt)[0]
    XIN, WP = be.dev(frame16(x, dt, in_pad)), be.dev(wp)
    B = be.dev(to16(np.asarray(b, np.float32), dt)[0]) if b is not None else None
    CB = be.dev(to16(np.asarray(cb, np.float32), dt)[0]) if cb is not None else None
    res_frame = frame16(res, dt, out_pad, SENTINEL) if res is not None else None
    RES = be.dev(res_frame) if res is not None else None
    OUT = be.dev(np.full((N, Ho + 2 * out_pad, Wo + 2 * out_pad, Cout), SENTINEL, np.uint16))
    d = _abi.Conv16Desc(in_=be.ptr(XIN), W=be.ptr(WP), out=be.ptr(OUT), bias=be.ptr(B), residual=be.ptr(RES), N=N, Hi=H, Wi=W, Cin=Cin, in_pad=in_pad, Ho=Ho, Wo=Wo,
                        Cout=Cout, out_pad=out_pad, KS=KS, stride=stride, pad_top=dpads[0], pad_left=dpads[1], upsample=up, dtype=DT[dt], chan_bias=be.ptr(CB))
    ok(be.lib.eegclip_conv16(d, be.stream))
    be.sync()
    got = be.host(OUT)
    assert border_is(got, out_pad, SENTINEL)
    if res is not None:
        assert np.array_equal(be.host(RES), res_frame)
    return unframe16(got, dt, out_pad), rpads


CONV_CASES = {
    # matrix-core forms (Cin % 64 == 0): M = N Ho Wo rows in 128-row tiles
    "3x3_two_m_tiles": dict(Cin=64, Cout=128, H=9, W=9),                                  # M = 162: the second tile partial
    "ext_res_cb": dict(Cin=64, Cout=192, H=9, W=8, res=1, cb=1),                          # the UNet's form, a masked N tile, two M tiles
    "1x1_res_three_m_tiles": dict(Cin=128, Cout=128, H=12, W=11, KS=1, res=1),
    "1x1_chunk2": dict(Cin=64, Cout=256, H=17, W=16, KS=1),                               # 10 tiles: chunk = 2, grid 16, idle workgroups, permuted tile walk
    "upsample": dict(Cin=64, Cout=128, H=5, W=7, up=1),
    "stride2_unet": dict(Cin=64, Cout=192, H=17, W=16, stride=2, pads=(1, 1)),
    "stride2_vae": dict(Cin=64, Cout=128, H=18, W=16, stride=2, pads=(0, 0)),             # bottom / right padding from the frame
    "out_pad0": dict(Cin=64, Cout=128, H=5, W=7, out_pad=0),
    "1x1_in_pad0": dict(Cin=64, Cout=128, H=5, W=7, KS=1, in_pad=0),
    "one_image": dict(Cin=64, Cout=128, H=5, W=7, N=1),
    # direct kernel
    "direct_4_16": dict(Cin=4, Cout=16, H=5, W=4),
    "direct_128_3": dict(Cin=128, Cout=3, H=6, W=5),                                      # 16-byte reads, odd Cout
    "direct_3_128": dict(Cin=3, Cout=128, H=6, W=5),                                      # scalar reads, odd Cin
    "direct_1x1_no_pads": dict(Cin=8, Cout=8, H=5, W=4, KS=1, in_pad=0, out_pad=0),
    "direct_512_8": dict(Cin=512, Cout=8, H=3, W=3),                                      # 72 KB of weights in LDS
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv16_per_element(be, name, dt):
    """|got - ref64| <= 0.5 ulp16(ref) + (K + 3) 2^-24 mag, K = KS^2 Cin, mag = the same convolution of |x|, |w| plus |bias| + |chan_bias| + |residual|: the
    fp32 dot-product bound (K products and K + 3 additions, each within 2^-24 relative of a partial result that mag dominates) plus the correctly rounded
    store.  Inputs are rounded to the dtype first, so the reference is exact for what the kernel reads"""
    case = CONV_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    Cin, Cout, H, W, N = case["Cin"], case["Cout"], case["H"], case["W"], case.get("N", 2)
    KS, stride, up = case.get("KS", 3), case.get("stride", 1), case.get("up", 0)
    K = KS * KS * Cin
    x = q16(rng.standard_normal((N, Cin, H, W)), dt)[1]
    w = q16(rng.standard_normal((Cout, Cin, KS, KS)) / K ** 0.5, dt)[1]
    b = q16(rng.standard_normal(Cout), dt)[1]
    rpads, _ = conv_geometry(KS, stride, up, case.get("pads", (0, 0)))
    ref = conv_ref(x, w, b, stride=stride, pads=rpads, up=bool(up))
    mag = conv_ref(np.abs(x), np.abs(w), np.abs(b), stride=stride, pads=rpads, up=bool(up))
    res = cb = None
    if case.get("cb"):
        cb = q16(rng.standard_normal((N, Cout)), dt)[1]
        ref, mag = ref + cb[:, :, None, None], mag + np.abs(cb)[:, :, None, None]
    if case.get("res"):
        res = q16(rng.standard_normal(ref.shape), dt)[1]
        ref, mag = ref + res, mag + np.abs(res)
    got, _ = run_conv16(be, dt, x, w, b, res, cb, KS, stride, up, case.get("pads", (0, 0)), case.get("in_pad", 1), case.get("out_pad", 1))
    assert got.shape == ref.shape and np.isfinite(got).all()
    bound = 0.5 * ulp16(ref, dt) + (K + 3) * 2.0 ** -24 * mag
    ratio = report(f"conv16 {name} {dt} {be.name}", float((np.abs(got - ref) / bound).max()))
    assert ratio <= 1.0, ratio


def distinct_weights(shape, dt, binades):
    """distinct normal numbers of the dtype per (co, tap, ci), from `binades` (a range of exponent fields), both signs.  16 bits do not hold the 128 * 9 * 64 =
    73 728 distinct values the matrix kernel's smallest 3 x 3 layer would need: element i takes value i % P of a shuffled pool, P the largest prime below the
    pool's size, so two elements with one value lie a multiple of P apart -- another output channel AND another input channel (checked for every such pair),
    which no mix-up of taps, of channels within a k-tile or of rows within a tile produces.  The direct kernel's 576 weights are all distinct"""
    Cout, KS, _, Cin = shape
    mant = 10 if dt == "f16" else 7
    pool = np.array([s | (e << mant) | m for s in (0, 0x8000) for e in binades for m in range(1 << mant)], np.uint16)
    P = next(p for p in range(len(pool), 1, -1) if all(p % d for d in range(2, int(p ** 0.5) + 1)))
    n = Cout * KS * KS * Cin
    for m in range(P, n, P):                                                 # every pair of elements (i - m, i) that shares a value
        i = np.arange(m, n)
        assert ((i // (KS * KS * Cin)) != ((i - m) // (KS * KS * Cin))).all() and ((i % Cin) != ((i - m) % Cin)).all()
    pool = np.random.default_rng(5).permutation(pool)[:P]
    bits = pool[np.arange(n) % P].reshape(shape)                             # (Cout, KS, KS, Cin): the kernel's [co][tap][ci] order
    return from16(bits, dt).astype(np.float64).transpose(0, 3, 1, 2)         # -> (Cout, Cin, KS, KS)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("form", ["plain", "upsample", "stride2"])
@pytest.mark.parametrize("kernel", ["matrix", "direct"])
def test_conv16_one_hot_address_map(be, kernel, form, dt):
    """one-hot input at a single (image, pixel, channel), no bias: every output is zero or one weight -- with upsampling the sum of the 1, 2 or 4 weights whose
    taps share the source pixel -- EXACTLY: a ky / kx exchange, an off-by-one in the upsampling's >> 1 or a channel swizzle of one operand fails outright,
    not within a tolerance.  For the sums the weights come from few enough binades (12 in fp16, 15 in bf16) that any four add exactly in fp32 in any order
    (lowest bit 2^(emin - mant), sum < 2^(emax + 3): 24 bits), so the stored value is the exact sum rounded to the dtype once"""
    Cin, Cout = (64, 128) if kernel == "matrix" else (4, 16)
    N, H, W = 2, 5, 6
    up, stride = int(form == "upsample"), 2 if form == "stride2" else 1
    x = np.zeros((N, Cin, H, W))
    x[1, Cin - 3, 3, 3 if stride == 2 else 2] = 1.0                          # stride 2, odd (y, x): the four corner taps; otherwise all nine
    if up:
        w = distinct_weights((Cout, 3, 3, Cin), dt, range(9, 21) if dt == "f16" else range(120, 135))
    else:
        w = distinct_weights((Cout, 3, 3, Cin), dt, range(1, 31) if dt == "f16" else range(1, 255))
    got, rpads = run_conv16(be, dt, x, w, None, None, None, 3, stride, up, (1, 1), 1, 1)
    ref = conv_ref(x, w, np.zeros(Cout), stride=stride, pads=rpads, up=bool(up))
    assert np.count_nonzero(conv_ref(x, np.abs(w), np.zeros(Cout), stride=stride, pads=rpads, up=bool(up))) == Cout * (4 if stride == 2 else 16 if up else 9)
    np.testing.assert_array_equal(got, q16(ref, dt)[1])


# ---------------------------------------------------------------------------------------------------------------------------------- groupnorm16

def gn_reference(x, g, b, G, eps):
    """fp64 GroupNorm of x (N, C, H, W): (ng = (x - mean) rstd gamma, mean (N, G), biased var (N, G), mean and rstd per channel (N, C, 1, 1))"""
    N, C, H, W = x.shape
    xg = x.reshape(N, G, -1)
    mean, var = xg.mean(2), xg.var(2)
    mean_c = np.repeat(mean, C // G, axis=1)[:, :, None, None]
    rstd_c = np.repeat(1.0 / np.sqrt(var + eps), C // G, axis=1)[:, :, None, None]
    return (x - mean_c) * rstd_c * g[None, :, None, None], mean, var, mean_c, rstd_c


def gn_two_pass_fp32(x, g, b, G, eps):
    """torch's arithmetic restated in fp32: mean, then the mean of squared deviations (no output rounding)"""
    N, C, H, W = x.shape
    xg = x.astype(np.float32).reshape(N, G, -1)
    mean = xg.mean(2, dtype=np.float32, keepdims=True)
    var = np.square(xg - mean).mean(2, dtype=np.float32, keepdims=True)
    y = ((xg - mean) * (np.float32(1) / np.sqrt(var + np.float32(eps)))).reshape(N, C, H, W)
    return (y * g.astype(np.float32)[None, :, None, None] + b.astype(np.float32)[None, :, None, None]).astype(np.float64)


def run_groupnorm16(be, dt, x, g, b, G, eps, silu, pad=1, out_pad=1, offset8=False, y_fill=SENTINEL):
    """-> (y (N, C, H, W) fp64, sums (N, G, 2)).  The input frame's border is NaN (only interior pixels count), the output frame's must stay as it was"""
    N, C, H, W = x.shape
    xf = frame16(x, dt, pad, SENTINEL)
    if offset8:                                                              # the same frame 8 bytes off a 16-byte boundary: the per-channel walk
        buf = np.zeros(xf.size + 8, np.uint16)
        buf[4:4 + xf.size] = xf.ravel()
        X = be.dev(buf)
        assert be.ptr(X) % 16 == 0
        xptr = be.ptr(X) + 8
    else:
        X = be.dev(xf)
        xptr = be.ptr(X)
    GA, BE = be.dev(to16(g.astype(np.float32), dt)[0]), be.dev(to16(b.astype(np.float32), dt)[0])
    Y = be.dev(np.full((N, H + 2 * out_pad, W + 2 * out_pad, C), y_fill, np.uint16))
    S = be.dev(np.full(N * G * 2, np.nan, np.float64))
    ok(be.lib.eegclip_groupnorm16(xptr, N, H, W, C, pad, G, be.ptr(GA), be.ptr(BE), eps, silu, be.ptr(Y), out_pad, be.ptr(S), DT[dt], be.stream))
    be.sync()
    got = be.host(Y)
    assert border_is(got, out_pad, y_fill)
    return unframe16(got, dt, out_pad), be.host(S).reshape(N, G, 2)


def gn_check(be, dt, label, x, g, b, G, silu, **kw):
    """bound per element, ng = (x - mean) rstd gamma:  ulp16(ref) + E,  E = 6e-5 (|ng| + |beta|) + 2^-22 |mean_g| rstd_g |gamma|  (one ulp of the stored
    value; fp32 arithmetic on the summands, as tests/test_kernels_unet.py::test_layernorm16_fp16_against_fp64; the fp32 rounding of the group mean, which
    moves every value of the group by 2^-25 |mean| rstd |gamma|).  With SiLU the same bound holds about ref = silu(v): ulp16(ref) + E, E still taken before
    the activation.
    `sums`: the mean from it within 2^-20 (|mean| + sd), the biased variance within 1.2e-4 relative (twice 6e-5: rstd = var^-1/2).
    -> (max err / bound, max relative error of the variance)"""
    eps = 1e-6
    ng, mean, var, mean_c, rstd_c = gn_reference(x, g, b, G, eps)
    beta = b[None, :, None, None]
    E = 6e-5 * (np.abs(ng) + np.abs(beta)) + 2.0 ** -22 * np.abs(mean_c) * rstd_c * np.abs(g)[None, :, None, None]
    pre = ng + beta
    # the inputs must leave a correct fp32 kernel room: torch's two-pass arithmetic within a quarter of the bound before output rounding
    self_ratio = float((np.abs(gn_two_pass_fp32(x, g, b, G, eps) - pre) / (ulp16(pre, dt) + E)).max())
    print(f"groupnorm16 {label} {dt}: fp32 two-pass restatement err / bound = {self_ratio:.3f}")
    assert self_ratio <= 0.25, self_ratio
    ref = pre / (1.0 + np.exp(-pre)) if silu else pre
    bound = ulp16(ref, dt) + E
    got, sums = run_groupnorm16(be, dt, x, g, b, G, eps, silu, **kw)
    n = x[0].size // G
    mean_k = sums[:, :, 0] / n
    var_k = sums[:, :, 1] / n - mean_k ** 2
    var_rel = float((np.abs(var_k - var) / var).max())
    mean_ratio = float((np.abs(mean_k - mean) / (2.0 ** -20 * (np.abs(mean) + np.sqrt(var)))).max())
    ratio = float((np.abs(got - ref) / bound).max()) if np.isfinite(got).all() else math.inf
    print(f"groupnorm16 {label} {dt} {be.name} silu={silu}: max err / bound = {ratio:.3f}, rel. error of var = {var_rel:.2e}, mean err / bound = {mean_ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert var_rel <= 1.2e-4, var_rel
    assert mean_ratio <= 1.0, mean_ratio
    return ratio, var_rel


def gn_inputs(rng, dt, N, C, H, W, mean=0.5, sd=2.0):
    x = q16(rng.standard_normal((N, C, H, W)) * sd + mean, dt)[1]
    return x, q16(1 + 0.2 * rng.standard_normal(C), dt)[1], q16(0.2 * rng.standard_normal(C), dt)[1]


GN_CASES = {
    "vector_two_blocks": dict(C=128, G=32, H=17, W=19),                                   # 323 pixels: two pixel blocks, the last one clipped
    "vector_idle_lanes": dict(C=512, G=32, H=3, W=3, N=1),                                # one image; 9 pixels in one clipped block
    "pairs_c2_apply": dict(C=320, G=32, H=17, W=19),                                      # pairs statistics, 2-channel apply
    "pairs_widest": dict(C=16384, G=32, H=1, W=2, N=1),                                   # the most channels the pairs form takes: 128 KB of LDS
    "pads_0_0": dict(C=64, G=16, H=5, W=6, pad=0, out_pad=0),
    "pads_1_0": dict(C=64, G=16, H=5, W=6, pad=1, out_pad=0),
    "pads_0_1": dict(C=64, G=16, H=5, W=6, pad=0, out_pad=1),
    "walk_offset8": dict(C=64, G=16, H=5, W=6, offset8=True),                             # x 8 bytes off 16: the per-channel walk
    "c12": dict(C=12, G=3, H=5, W=6),                                                     # C % 8 != 0
    "c24": dict(C=24, G=2, H=5, W=6),
    "walk_513_groups": dict(C=2052, G=513, H=1, W=2, N=1),                                # the walk's LDS table of more groups than the vector form's partials
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm16_per_element(be, name, silu, dt):
    case = dict(GN_CASES[name])
    rng = np.random.default_rng(sum(map(ord, name)))
    C, G, H, W, N = case.pop("C"), case.pop("G"), case.pop("H"), case.pop("W"), case.pop("N", 2)
    x, g, b = gn_inputs(rng, dt, N, C, H, W)
    gn_check(be, dt, name, x, g, b, G, silu, y_fill=SENTINEL if silu else 0, **case)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,ratio", [(128, 0.25), (128, 16), (128, 64), (128, 160), (128, 400), (128, -0.25), (128, -16), (128, -64), (128, -160), (128, -400),
                                     (320, 64)])
def test_groupnorm16_large_mean(be, C, ratio, dt):
    """a group whose |mean| is `ratio` standard deviations: sums of x and x^2 kept in fp32 lose the variance (sum x^2 / n - mean^2 cancels ratio^2 of its
    digits); the statistics kernels sum about a pivot instead"""
    rng = np.random.default_rng(int(ratio * 4) + 2000 + C)
    x, g, b = gn_inputs(rng, dt, 2, C, 17, 19, mean=ratio * 0.25, sd=0.25)
    gn_check(be, dt, f"C={C} mean/sd={ratio}", x, g, b, 32, 0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("C,G,H,W,offset8", [(128, 32, 17, 19, False), (320, 32, 17, 19, False), (64, 16, 5, 6, True)])
def test_groupnorm16_constant_groups(be, C, G, H, W, offset8, dt):
    """every group constant: var = 0, rstd = eps^-1/2 = 1000 multiplies whatever the mean is off by; the output is beta within one ulp, no NaN"""
    rng = np.random.default_rng(C)
    N = 2
    c = q16(rng.standard_normal((N, G)) * 2 + 0.5, dt)[1]
    x = np.broadcast_to(np.repeat(c, C // G, axis=1)[:, :, None, None], (N, C, H, W)).copy()
    _, g, b = gn_inputs(rng, dt, N, C, H, W)
    got, sums = run_groupnorm16(be, dt, x, g, b, G, 1e-6, 0, offset8=offset8)
    assert np.isfinite(got).all() and np.isfinite(sums).all()
    beta = np.broadcast_to(b[None, :, None, None], got.shape)
    ratio = report(f"groupnorm16 constant groups C={C} {dt} {be.name} (err / ulp)", float((np.abs(got - beta) / ulp16(beta, dt)).max()))
    assert ratio <= 1.0, ratio


def test_groupnorm16_refusals(be):
    """N * groups > 4096 (the apply kernel's LDS table) and an odd channel count per group; every buffer has its full size"""
    for N, C, G in [(129, 64, 32), (2, 24, 8)]:
        X, GA, BE = be.dev(np.zeros((N, 1, 1, C), np.uint16)), be.dev(np.zeros(C, np.uint16)), be.dev(np.zeros(C, np.uint16))
        Y, S = be.dev(np.zeros((N, 1, 1, C), np.uint16)), be.dev(np.zeros(N * G * 2, np.float64))
        for dt in DTS:
            assert be.lib.eegclip_groupnorm16(be.ptr(X), N, 1, 1, C, 0, G, be.ptr(GA), be.ptr(BE), 1e-6, 0, be.ptr(Y), 0, be.ptr(S), DT[dt], be.stream) < 0
    be.sync()


# ------------------------------------------------------------------------------------------------------------------- the small elementwise kernels

@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,cols,ld", [(5, 200, 200), (5, 300, 320), (3, 1024, 1024), (2, 1, 8)])
def test_softmax_rows16_per_element(be, rows, cols, ld, dt):
    """0.5 ulp16(ref) + 1e-5 ref: the rounded store plus ~forty fp32 epsilons at |z| ~ 4 for expf and the row sum.  Row 0 holds equal values; the last row (if
    wide enough) holds entries near +-60000, where the scaled logits span 30000 and fp16 is about to overflow.  Columns cols .. ld stay bit-unchanged"""
    rng = np.random.default_rng(rows * cols + ld)
    scale = 0.25
    s = rng.standard_normal((rows, cols)) * 3
    s[0] = 1.75
    if cols >= 200:
        s[-1, ::3] = 60000 - 32 * rng.integers(0, 4, s[-1, ::3].shape)
        s[-1, 1::3] = -60000 + 32 * rng.integers(0, 4, s[-1, 1::3].shape)
    bits, s = q16(s, dt)
    buf = rng.integers(0, 1 << 16, (rows, ld)).astype(np.uint16)
    buf[:, :cols] = bits
    SM = be.dev(buf)
    ok(be.lib.eegclip_softmax_rows16(be.ptr(SM), rows, cols, ld, scale, DT[dt], be.stream))
    be.sync()
    out = be.host(SM)
    assert np.array_equal(out[:, cols:], buf[:, cols:])
    got = from16(out[:, :cols], dt).astype(np.float64)
    z = scale * s
    e = np.exp(z - z.max(1, keepdims=True))
    ref = e / e.sum(1, keepdims=True)
    bound = 0.5 * ulp16(ref, dt) + 1e-5 * ref
    ratio = report(f"softmax_rows16 {rows}x{cols} ld={ld} {dt} {be.name}", float((np.abs(got - ref) / bound).max()))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("dt", DTS)
def test_vae_sample16_per_element(be, dt):
    """z = mean + exp(0.5 clamp(logvar, -30, 20)) noise within 0.5 ulp16 + 1e-5 (|mean| + |sigma noise|); both clamp ends decide the stored value (logvar 50:
    sigma = e^10, not e^25; logvar -40 over a zero mean: e^-15, not e^-20); without noise the mean comes back bit for bit"""
    rng = np.random.default_rng(11)
    P, L = 7, 4
    mom, nz = rng.standard_normal((P, 2 * L)), np.clip(rng.standard_normal((P, L)), -2, 2)
    mom[0, L:] = 50.0
    mom[1, L:], mom[1, :L] = -40.0, 0.0
    (mbits, mom), (nbits, nz) = q16(mom, dt), q16(nz, dt)
    M, NZ, Z = be.dev(mbits), be.dev(nbits), be.dev(np.full((P, L), SENTINEL, np.uint16))
    ok(be.lib.eegclip_vae_sample16(be.ptr(M), be.ptr(NZ), be.ptr(Z), P, L, DT[dt], be.stream))
    be.sync()
    got = from16(be.host(Z), dt).astype(np.float64)
    sn = np.exp(0.5 * np.clip(mom[:, L:], -30, 20)) * nz
    ref = mom[:, :L] + sn
    bound = 0.5 * ulp16(ref, dt) + 1e-5 * (np.abs(mom[:, :L]) + np.abs(sn))
    ratio = report(f"vae_sample16 {dt} {be.name}", float((np.abs(got - ref) / bound).max()))
    assert ratio <= 1.0, ratio
    ok(be.lib.eegclip_vae_sample16(be.ptr(M), None, be.ptr(Z), P, L, DT[dt], be.stream))
    be.sync()
    np.testing.assert_array_equal(be.host(Z), mbits[:, :L])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,D", [(5, 320), (1, 8)])
def test_geglu16_per_element(be, M, D, dt):
    """a gelu(g) (erf form) within 0.5 ulp16 + 1e-5 |a|"""
    rng = np.random.default_rng(M + D)
    bits, x = q16(rng.standard_normal((M, 2 * D)) * 2, dt)
    X, Y = be.dev(bits), be.dev(np.full((M, D), SENTINEL, np.uint16))
    ok(be.lib.eegclip_geglu16(be.ptr(X), be.ptr(Y), M, D, DT[dt], be.stream))
    be.sync()
    got = from16(be.host(Y), dt).astype(np.float64)
    a, g = x[:, :D], x[:, D:]
    ref = a * 0.5 * g * (1 + np.vectorize(math.erf)(g / math.sqrt(2)))
    bound = 0.5 * ulp16(ref, dt) + 1e-5 * np.abs(a)
    ratio = report(f"geglu16 {M}x{D} {dt} {be.name}", float((np.abs(got - ref) / bound).max()))
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pad,out_pad", [(0, 0), (1, 1)])
@pytest.mark.parametrize("Ca,Cb", [(64, 320), (8, 24)])
def test_concat16_exact(be, Ca, Cb, pad, out_pad, dt):
    rng = np.random.default_rng(Ca + Cb)
    N, H, W = 2, 3, 4
    a, b = q16(rng.standard_normal((N, Ca, H, W)), dt)[1], q16(rng.standard_normal((N, Cb, H, W)), dt)[1]
    A, B = be.dev(frame16(a, dt, pad, SENTINEL)), be.dev(frame16(b, dt, pad, SENTINEL))
    OUT = be.dev(np.full((N, H + 2 * out_pad, W + 2 * out_pad, Ca + Cb), SENTINEL, np.uint16))
    ok(be.lib.eegclip_concat16(be.ptr(A), be.ptr(B), be.ptr(OUT), N, H, W, pad, Ca, Cb, out_pad, DT[dt], be.stream))
    be.sync()
    got = be.host(OUT)
    np.testing.assert_array_equal(unframe16(got, dt, out_pad), np.concatenate([a, b], 1))
    assert border_is(got, out_pad, SENTINEL)
