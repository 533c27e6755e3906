"""csrc/convt16.hip (ConvTranspose2d, kernel 4, stride 2, padding 1, on padded NHWC frames) through the C ABI on both backends, against numpy fp64 on the
16-bit-rounded inputs.  The reference is the SCATTER definition of the transposed convolution (out[2y - 1 + ky][2x - 1 + kx] += in[y][x] w[ky][kx]), not the
sub-pixel phase form the kernel runs.

Bound, from the arithmetic (u = half an ulp of the 16-bit format relative to 1: 2^-11 for fp16, 2^-8 for bf16): every product of two 16-bit factors is exact
in fp32; at most 4 Cin of them reach an output element and are summed in fp32 in some order, then y = acc * scale + shift (two fp32 roundings) and one
rounding to 16 bit:
    |error| <= |scale| (4 Cin + 2) 2^-24 sum|a w|  +  2^-23 |y|  +  u |y|  +  the smallest subnormal of the format
ReLU is 1-Lipschitz and is applied to the reference too, so the bound of y holds after it.

Worst |error| / bound over every case and epilogue below, emulator and MI355X alike: fp16 0.923, bf16 0.980 -- the half-ulp term of the final rounding (a
result just above a power of two uses all of u |y|); the fp32 terms are three orders smaller.
"""
import numpy as np
import pytest

from backends import be, byref, ok  # noqa: F401
from eeg_image_decode_amd import _abi
from test_kernels_gemm16 import DT, from16, to16

SENT = 0x7BCD                          # a finite 16-bit pattern in both dtypes
U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133}
EINVAL, EALIGN = -1, -2
WORST = {}
KY = ((1, 3), (2, 0))                  # [phase half][tap half] -> kernel index along that axis

# (N, Hi, Wi, Cin, Cout)
CASES = [(1, 1, 1, 128, 64), (3, 1, 1, 192, 32), (2, 2, 2, 64, 128), (2, 3, 5, 64, 64), (1, 9, 15, 64, 48), (17, 1, 1, 64, 16), (1, 8, 8, 64, 4),
         (2, 4, 4, 128, 4)]


def pack(w):
    """torch's (Cin, Cout, 4, 4) -> [phase 2 py + px][Cout][tap 2 ty + tx][Cin]"""
    Cin, Cout = w.shape[:2]
    p = np.empty((4, Cout, 4, Cin), w.dtype)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    p[2 * py + px, :, 2 * ty + tx, :] = w[:, :, KY[py][ty], KY[px][tx]].T
    return p


def scatter_ref(x, w):
    """x (N, Cin, H, W), w (Cin, Cout, 4, 4) float64 -> (N, Cout, 2H, 2W): conv_transpose2d(x, w, stride=2, padding=1) by its definition"""
    N, _, H, W = x.shape
    buf = np.zeros((N, w.shape[1], 2 * H + 2, 2 * W + 2))
    for ky in range(4):
        for kx in range(4):
            buf[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.einsum("nchw,cd->ndhw", x, w[:, :, ky, kx])     # row 2y - 1 + ky, held at index + 1
    return buf[:, :, 1:2 * H + 1, 1:2 * W + 1]


def live_mask(Hi, Wi):
    m = 0
    for phase in range(4):
        for tap in range(4):
            if not ((tap >> 1) and Hi == 1) and not ((tap & 1) and Wi == 1):
                m |= 1 << (4 * phase + tap)
    return m


def desc(be, X, W, out, N, Hi, Wi, Cin, Cout, dt, scale=None, shift=None, relu=0, mask=0xFFFF, **over):
    f = dict(in_=be.ptr(X), W=be.ptr(W), out=be.ptr(out), scale=be.ptr(scale), shift=be.ptr(shift), N=N, Hi=Hi, Wi=Wi, Cin=Cin, Ho=2 * Hi, Wo=2 * Wi, Cout=Cout,
             KS=4, stride=2, pad=1, relu=relu, tap_mask=mask, dtype=DT[dt])
    f.update(over)
    return _abi.Convt16Desc(**f)


def fresh_out(be, N, Hi, Wi, Cout, extra=3):
    """the output buffer before a launch: zero border, sentinel interior, `extra` sentinel rows behind the frame; (buffer, frame elements)"""
    Ho, Wo = 2 * Hi, 2 * Wi
    if Cout >= 16:
        fr = np.zeros((N, Ho + 2, Wo + 2, Cout), np.uint16)
        fr[:, 1:-1, 1:-1] = SENT
    else:
        fr = np.full((N, Cout, Ho, Wo), SENT, np.uint16)
    flat = np.concatenate([fr.ravel(), np.full(extra * (Wo + 2) * Cout, SENT, np.uint16)])
    return be.dev(flat), fr.size


def run(be, d, out, N, Hi, Wi, Cout, nframe):
    """launch, check the layout, return the result bits as (N, Cout, Ho, Wo)"""
    ok(be.lib.eegclip_convt16(byref(d), be.stream))
    be.sync()
    raw = be.host(out)
    assert (raw[nframe:] == SENT).all(), "rows behind the frame were written"
    Ho, Wo = 2 * Hi, 2 * Wi
    if Cout >= 16:
        fr = raw[:nframe].reshape(N, Ho + 2, Wo + 2, Cout)
        assert not fr[:, 0].any() and not fr[:, -1].any() and not fr[:, :, 0].any() and not fr[:, :, -1].any(), "the frame's border was written"
        got = fr[:, 1:-1, 1:-1].transpose(0, 3, 1, 2)
    else:
        got = raw[:nframe].reshape(N, Cout, Ho, Wo)
    assert (got != SENT).all(), "an interior element was left unwritten"
    return np.ascontiguousarray(got)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("N,Hi,Wi,Cin,Cout", CASES)
def test_convt16(be, N, Hi, Wi, Cin, Cout, dt):
    """every epilogue (scale / shift given or NULL, ReLU on or off) against the scatter reference; layout; two runs bit-identical; the dead-tap mask gives the
    bits of the all-taps mask"""
    rng = np.random.default_rng(1000 * N + 100 * Hi + 10 * Wi + Cin + Cout)
    x16, x = to16(rng.standard_normal((N, Hi, Wi, Cin)).astype(np.float32), dt)
    w16, w = to16((rng.standard_normal((Cin, Cout, 4, 4)) / np.sqrt(4 * Cin)).astype(np.float32), dt)
    scale = (rng.uniform(0.5, 1.5, Cout) * rng.choice([-1.0, 1.0], Cout)).astype(np.float32)
    shift = rng.standard_normal(Cout).astype(np.float32)
    frame = np.zeros((N, Hi + 2, Wi + 2, Cin), np.uint16)
    frame[:, 1:-1, 1:-1] = x16
    X, W, S, T = be.dev(frame), be.dev(pack(w16)), be.dev(scale), be.dev(shift)
    x64, w64 = x.astype(np.float64).transpose(0, 3, 1, 2), w.astype(np.float64)
    acc, mag = scatter_ref(x64, w64), scatter_ref(np.abs(x64), np.abs(w64))
    worst = 0.0
    for use_affine in (False, True):
        sc = scale.astype(np.float64)[None, :, None, None] if use_affine else 1.0
        sh = shift.astype(np.float64)[None, :, None, None] if use_affine else 0.0
        y = acc * sc + sh
        bound = np.abs(sc) * (4 * Cin + 2) * 2.0 ** -24 * mag + 2.0 ** -23 * np.abs(y) + U[dt] * np.abs(y) + TINY[dt]
        for relu in (0, 1):
            ref = np.maximum(y, 0.0) if relu else y
            out, nframe = fresh_out(be, N, Hi, Wi, Cout)
            d = desc(be, X, W, out, N, Hi, Wi, Cin, Cout, dt, S if use_affine else None, T if use_affine else None, relu)
            bits = run(be, d, out, N, Hi, Wi, Cout, nframe)
            got = from16(bits, dt).astype(np.float64)
            assert np.isfinite(got).all()
            ratio = float((np.abs(got - ref) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (use_affine, relu, ratio)
            if relu:
                assert (got >= 0).all() and (got == 0).any() and (got > 0).any()
            out2, _ = fresh_out(be, N, Hi, Wi, Cout)
            again = run(be, desc(be, X, W, out2, N, Hi, Wi, Cin, Cout, dt, S if use_affine else None, T if use_affine else None, relu), out2, N, Hi, Wi, Cout, nframe)
            assert np.array_equal(again, bits), "two runs differ"
            if live_mask(Hi, Wi) != 0xFFFF:
                out3, _ = fresh_out(be, N, Hi, Wi, Cout)
                dm = desc(be, X, W, out3, N, Hi, Wi, Cin, Cout, dt, S if use_affine else None, T if use_affine else None, relu, mask=live_mask(Hi, Wi))
                assert np.array_equal(run(be, dm, out3, N, Hi, Wi, Cout, nframe), bits), "the dead-tap mask changes the result"
    WORST[(be.name, dt)] = max(WORST.get((be.name, dt), 0.0), worst)
    print(f"convt16 {be.name} N={N} {Hi}x{Wi} {Cin}->{Cout} {dt}: worst |error| / bound {worst:.3f} (over all cases so far {WORST[(be.name, dt)]:.3f})")


def test_convt16_dead_taps_are_not_read(be):
    """1 x 1 with the dead-tap mask: the weights of the three dead taps of every phase are NaN and must not reach the output"""
    N, Cin, Cout, dt = 2, 64, 32, "f16"
    rng = np.random.default_rng(5)
    x16, _ = to16(rng.standard_normal((N, 1, 1, Cin)).astype(np.float32), dt)
    w16, _ = to16((rng.standard_normal((Cin, Cout, 4, 4)) / 16).astype(np.float32), dt)
    frame = np.zeros((N, 3, 3, Cin), np.uint16)
    frame[:, 1:-1, 1:-1] = x16
    p = pack(w16)
    poisoned = p.copy()
    poisoned[:, :, 1:, :] = 0x7E00
    X = be.dev(frame)
    res = []
    for wts in (p, poisoned):
        out, nframe = fresh_out(be, N, 1, 1, Cout)
        W = be.dev(wts)
        res.append(run(be, desc(be, X, W, out, N, 1, 1, Cin, Cout, dt, mask=0x1111), out, N, 1, 1, Cout, nframe))
    assert np.isfinite(from16(res[1], dt)).all() and np.array_equal(res[0], res[1])


def test_convt16_rejections(be):
    N, Hi, Wi, Cin, Cout = 1, 2, 2, 128, 32
    X = be.zeros((N, Hi + 2, Wi + 2, Cin + 8), np.uint16)
    W = be.zeros((4, Cout, 4, Cin), np.uint16)
    out = be.zeros((N, 2 * Hi + 2, 2 * Wi + 2, Cout), np.uint16)

    def f(dt="f16", mask=0xFFFF, Hi_=Hi, Wi_=Wi, Cin_=Cin, Cout_=Cout, **over):
        d = desc(be, X, W, out, N, Hi_, Wi_, Cin_, Cout_, dt, mask=mask)
        for k, v in over.items():
            setattr(d, k, v)
        return be.lib.eegclip_convt16(byref(d), be.stream)

    assert f() == 0
    assert f(Cin_=96) == EINVAL                                         # Cin % 64
    assert f(in_=be.ptr(X) + 2) == EALIGN and f(W=be.ptr(W) + 8) == EALIGN
    assert f(Ho=2 * Hi + 1) == EINVAL and f(Wo=Wi) == EINVAL
    assert f(KS=3) == EINVAL and f(stride=1) == EINVAL and f(pad=0) == EINVAL
    assert f(Cout_=24) == EINVAL                                        # neither < 16 nor a multiple of 16
    assert f(Cout_=8, Cin_=320) == EINVAL                               # the direct form's weights beyond its LDS
    assert f(mask=0x1111) == EINVAL and f(mask=0xFFFE) == EINVAL        # 2 x 2: every tap is live
    assert f(mask=0x1FFFF) == EINVAL
    assert f(Hi_=1, Wi_=1, mask=0x1111) == 0 and f(Hi_=1, Wi_=1, mask=0x1110) == EINVAL
    assert f(Hi_=1, Wi_=2, mask=0x3333) == 0 and f(Hi_=1, Wi_=2, mask=0x1111) == EINVAL
    assert f(dtype=5) == EINVAL and f(relu=2) == EINVAL and f(in_=None) == EINVAL
    assert be.lib.eegclip_convt16(None, be.stream) == EINVAL
    be.sync()
