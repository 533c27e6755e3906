"""csrc/convt16_bwd.hip (the backward of ConvTranspose2d(4, 2, 1) on padded NHWC frames, and the training-time weight packing) through the C ABI on both backends,
against numpy fp64 on the 16-bit-rounded inputs.  References, from the definitions: the data gradient is the ADJOINT of test_kernels_convt16.scatter_ref (the test
checks <scatter_ref(x, w), dz> == <x, dx_ref> itself), the weight gradient the plain sum over pixels of x[ci] dz[co] at the scattered position, db the sum of dz.

Bounds, from the arithmetic (u = half an ulp of the 16-bit format relative to 1):
  bwd_data, matrix-core form    products of two 16-bit factors are exact in fp32; 16 Cout of them are summed in fp32 in some order, then one rounding to 16 bit:
                                |error| <= 16 Cout 2^-24 sum|dz w| + u |dx| + the smallest subnormal.
  bwd_data, direct form         dz is fp32: each product is rounded once more -> (16 Cout + 1) 2^-24 sum|dz w| + u |dx| + the smallest subnormal.
  bwd_weight                    M = N Hi Wi products (exact, or rounded once in the direct form), summed in fp32 in some order within a slab, then the slabs; the
                                division by the power-of-two loss scale is exact; fp32 out, no 16-bit rounding: |error| <= (M + slabs + 1) 2^-24 sum|x dz| / scale.
  db                            4 M values of dz (the taps ky, kx in {1, 2}) and one partial row per slab: (4 M + 2 slabs + 1) 2^-24 sum|dz| / scale bounds it.
Worst |error| / bound over every case below (printed per case with `pytest -s`): bwd_data fp16 0.956, bf16 0.988 on the emulator and the MI355X alike (the half-ulp
term of the final rounding); bwd_weight dW fp16 0.385 / bf16 0.269 on the emulator, 0.355 / 0.253 on the MI355X (the matrix cores add in another order), db 0.004 /
0.002 on both (a worst-case sum bound is far from a random sum's error).
"""
import numpy as np
import pytest

from backends import be, byref, ok  # noqa: F401
from eeg_image_decode_amd import _abi
from test_kernels_convt16 import SENT, TINY, U, pack, scatter_ref
from test_kernels_gemm16 import DT, from16, to16

EINVAL, EALIGN = -1, -2
NAN16 = 0x7E00
WORST = {}

# (N, Hi, Wi, Cin, Cout)
CASES = [(1, 1, 1, 128, 64), (3, 1, 1, 192, 64), (17, 1, 1, 64, 64), (2, 2, 2, 64, 128), (2, 3, 5, 64, 64), (1, 9, 15, 64, 64), (1, 8, 8, 64, 4), (2, 4, 4, 128, 4)]


def live_mask(Hi, Wi):
    """bit 4 ky + kx: the taps that meet the interior of dz for some pixel"""
    return sum(1 << (4 * ky + kx) for ky in range(4) for kx in range(4) if not (ky in (0, 3) and Hi == 1) and not (kx in (0, 3) and Wi == 1))


def pad1(a):
    return np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))


def bwd_data_ref(dz, w, H, W):
    """dz (N, Cout, 2H, 2W), w (Cin, Cout, 4, 4) float64 -> dx (N, Cin, H, W): dx[y][x] = sum dz[2y - 1 + ky][2x - 1 + kx] w[ky][kx]"""
    zp = pad1(dz)
    dx = np.zeros((dz.shape[0], w.shape[0], H, W))
    for ky in range(4):
        for kx in range(4):
            dx += np.einsum("ndhw,cd->nchw", zp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2], w[:, :, ky, kx])
    return dx


def bwd_weight_ref(x, dz):
    """x (N, Cin, H, W), dz (N, Cout, 2H, 2W) float64 -> dW (Cin, Cout, 4, 4)"""
    H, W = x.shape[2:]
    zp = pad1(dz)
    dW = np.zeros((x.shape[1], dz.shape[1], 4, 4))
    for ky in range(4):
        for kx in range(4):
            dW[:, :, ky, kx] = np.einsum("nchw,ndhw->cd", x, zp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2])
    return dW


def frame_of(bits_nhwc):
    N, H, W, C = bits_nhwc.shape
    fr = np.zeros((N, H + 2, W + 2, C), np.uint16)
    fr[:, 1:-1, 1:-1] = bits_nhwc
    return fr


def make_dz(rng, N, Hi, Wi, Cout, dt):
    """(device operand, float64 NCHW values): a 16-bit padded NHWC frame for the matrix-core forms, unpadded fp32 NCHW for the direct forms"""
    if Cout >= 16:
        z16, z = to16(rng.standard_normal((N, 2 * Hi, 2 * Wi, Cout)).astype(np.float32), dt)
        return frame_of(z16), z.astype(np.float64).transpose(0, 3, 1, 2)
    z = rng.standard_normal((N, Cout, 2 * Hi, 2 * Wi)).astype(np.float32)
    return z, z.astype(np.float64)


def note(kind, be, dt, ratio):
    WORST[(kind, be.name, dt)] = max(WORST.get((kind, be.name, dt), 0.0), ratio)
    return WORST[(kind, be.name, dt)]


# ---------------------------------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("Cin,Cout", sorted({(c[3], c[4]) for c in CASES} | {(64, 48), (64, 3)}))
def test_pack_train(be, Cin, Cout, dt):
    """the forward packing is bit-equal to pack() of the rounded weight, the data-gradient packing is [Cin][4 ky + kx][Cout]; nothing behind either is written"""
    rng = np.random.default_rng(Cin + Cout)
    w32 = (rng.standard_normal((Cin, Cout, 4, 4)) / np.sqrt(4 * Cin)).astype(np.float32)
    w16, _ = to16(w32, dt)
    n = Cin * Cout * 16
    F, B = be.dev(np.full(n + 64, SENT, np.uint16)), be.dev(np.full(n + 64, SENT, np.uint16))
    W = be.dev(w32)
    ok(be.lib.eegclip_convt16_pack_train(be.ptr(W), be.ptr(F), be.ptr(B), Cin, Cout, DT[dt], be.stream))
    be.sync()
    f, b = be.host(F), be.host(B)
    assert (f[n:] == SENT).all() and (b[n:] == SENT).all()
    assert np.array_equal(f[:n].reshape(4, Cout, 4, Cin), pack(w16))
    assert np.array_equal(b[:n].reshape(Cin, 16, Cout), w16.reshape(Cin, Cout, 16).transpose(0, 2, 1))


def test_pack_train_rejections(be):
    W, F, B = be.zeros((64, 32, 4, 4)), be.zeros(64 * 32 * 16, np.uint16), be.zeros(64 * 32 * 16, np.uint16)
    f = lambda w=be.ptr(W), a=be.ptr(F), b=be.ptr(B), Cin=64, Cout=32, dt=1: be.lib.eegclip_convt16_pack_train(w, a, b, Cin, Cout, dt, be.stream)   # noqa: E731
    assert f() == 0
    assert f(Cin=96) == EINVAL and f(Cout=0) == EINVAL and f(Cout=24) == EINVAL and f(dt=3) == EINVAL and f(w=None) == EINVAL and f(b=None) == EINVAL
    assert f(w=be.ptr(W) + 4) == EALIGN and f(a=be.ptr(F) + 2) == EALIGN
    be.sync()


# ---------------------------------------------------------------------------------------------------------------------------------------- data gradient
def dx_buffer(be, N, Hi, Wi, Cin, extra=3):
    fr = np.zeros((N, Hi + 2, Wi + 2, Cin), np.uint16)
    fr[:, 1:-1, 1:-1] = SENT
    return be.dev(np.concatenate([fr.ravel(), np.full(extra * (Wi + 2) * Cin, SENT, np.uint16)])), fr.size


def run_data(be, Z, Wb, N, Hi, Wi, Cin, Cout, dt, mask=0xFFFF):
    out, nframe = dx_buffer(be, N, Hi, Wi, Cin)
    d = _abi.Convt16BwdDataDesc(dz=be.ptr(Z), W=be.ptr(Wb), dx=be.ptr(out), N=N, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, tap_mask=mask, dtype=DT[dt])
    ok(be.lib.eegclip_convt16_bwd_data(byref(d), be.stream))
    be.sync()
    raw = be.host(out)
    assert (raw[nframe:] == SENT).all(), "rows behind the frame were written"
    fr = raw[:nframe].reshape(N, Hi + 2, Wi + 2, Cin)
    assert not fr[:, 0].any() and not fr[:, -1].any() and not fr[:, :, 0].any() and not fr[:, :, -1].any(), "the frame's border was written"
    got = fr[:, 1:-1, 1:-1]
    assert (got != SENT).all(), "an interior element was left unwritten"
    return np.ascontiguousarray(got.transpose(0, 3, 1, 2))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("N,Hi,Wi,Cin,Cout", CASES)
def test_bwd_data(be, N, Hi, Wi, Cin, Cout, dt):
    rng = np.random.default_rng(1000 * N + 100 * Hi + 10 * Wi + Cin + Cout)
    w16, w = to16((rng.standard_normal((Cin, Cout, 4, 4)) / np.sqrt(4 * Cout)).astype(np.float32), dt)
    zdev, z64 = make_dz(rng, N, Hi, Wi, Cout, dt)
    w64 = w.astype(np.float64)
    ref, mag = bwd_data_ref(z64, w64, Hi, Wi), bwd_data_ref(np.abs(z64), np.abs(w64), Hi, Wi)
    xr = rng.standard_normal((N, Cin, Hi, Wi))                                       # the reference IS the adjoint of the forward's definition
    lhs, rhs = float((scatter_ref(xr, w64) * z64).sum()), float((xr * ref).sum())
    assert abs(lhs - rhs) <= 1e-10 * float((np.abs(xr) * mag).sum())
    Z, Wb = be.dev(zdev), be.dev(np.ascontiguousarray(w16.reshape(Cin, Cout, 16).transpose(0, 2, 1)))
    bits = run_data(be, Z, Wb, N, Hi, Wi, Cin, Cout, dt)
    got = from16(bits, dt).astype(np.float64)
    assert np.isfinite(got).all()
    bound = (16 * Cout + (Cout < 16)) * 2.0 ** -24 * mag + U[dt] * np.abs(ref) + TINY[dt]
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"convt16_bwd_data {be.name} N={N} {Hi}x{Wi} {Cin}<-{Cout} {dt}: worst |error| / bound {ratio:.3f} (so far {note('data', be, dt, ratio):.3f})")
    assert ratio <= 1.0
    assert np.array_equal(run_data(be, Z, Wb, N, Hi, Wi, Cin, Cout, dt), bits), "two runs differ"
    if live_mask(Hi, Wi) != 0xFFFF:
        assert np.array_equal(run_data(be, Z, Wb, N, Hi, Wi, Cin, Cout, dt, mask=live_mask(Hi, Wi)), bits), "the dead-tap mask changes the result"


def test_bwd_data_dead_taps_are_not_read(be):
    """1 x 1 with the dead-tap mask: the weights of the twelve dead taps are NaN and must not reach dx"""
    N, Cin, Cout, dt = 2, 64, 64, "f16"
    rng = np.random.default_rng(5)
    w16, _ = to16((rng.standard_normal((Cin, 16, Cout)) / 16).astype(np.float32), dt)
    zdev, _ = make_dz(rng, N, 1, 1, Cout, dt)
    poisoned = w16.copy()
    poisoned[:, [k for k in range(16) if not (live_mask(1, 1) >> k) & 1], :] = NAN16
    Z = be.dev(zdev)
    res = [run_data(be, Z, be.dev(wts), N, 1, 1, Cin, Cout, dt, mask=live_mask(1, 1)) for wts in (w16, poisoned)]
    assert live_mask(1, 1) == 0x0660 and np.isfinite(from16(res[1], dt)).all() and np.array_equal(res[0], res[1])


def test_bwd_data_rejections(be):
    N, Hi, Wi, Cin, Cout = 1, 2, 2, 128, 64
    Z = be.zeros((N, 2 * Hi + 2, 2 * Wi + 2, Cout + 8), np.uint16)
    W = be.zeros((Cin, 16, Cout + 8), np.uint16)
    out = be.zeros((N, Hi + 2, Wi + 2, Cin), np.uint16)

    def f(**over):
        kw = dict(dz=be.ptr(Z), W=be.ptr(W), dx=be.ptr(out), N=N, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, tap_mask=0xFFFF, dtype=1)
        kw.update(over)
        return be.lib.eegclip_convt16_bwd_data(byref(_abi.Convt16BwdDataDesc(**kw)), be.stream)

    assert f() == 0
    assert f(Cin=96) == EINVAL and f(Cout=32) == EINVAL and f(Cout=96) == EINVAL and f(N=0) == EINVAL and f(Hi=0) == EINVAL
    assert f(Cout=8, Cin=320) == EINVAL                                 # the direct form's weights beyond its LDS
    assert f(dz=be.ptr(Z) + 2) == EALIGN and f(W=be.ptr(W) + 8) == EALIGN and f(dx=be.ptr(out) + 1) == EALIGN
    assert f(tap_mask=0x0660) == EINVAL and f(tap_mask=0xFFFE) == EINVAL and f(tap_mask=0x1FFFF) == EINVAL          # 2 x 2: every tap is live
    assert f(Hi=1, Wi=1, tap_mask=0x0660) == 0 and f(Hi=1, Wi=1, tap_mask=0x0640) == EINVAL
    assert f(Hi=1, Wi=2, tap_mask=0x0FF0) == 0 and f(Hi=1, Wi=2, tap_mask=0x0660) == EINVAL
    assert f(dtype=5) == EINVAL and f(dz=None) == EINVAL and f(dx=None) == EINVAL
    assert be.lib.eegclip_convt16_bwd_data(None, be.stream) == EINVAL
    be.sync()


# ---------------------------------------------------------------------------------------------------------------------------------------- weight gradient
FSENT = np.float32(-12345.5)


def run_weight(be, X, Z, N, Hi, Wi, Cin, Cout, dt, slabs, scale):
    nws = be.lib.eegclip_convt16_bwd_weight_workspace_floats(N, Hi, Wi, Cin, Cout, slabs)
    assert nws > 0
    n = Cin * Cout * 16
    dW, db, ws = be.dev(np.full(n + 16, FSENT, np.float32)), be.dev(np.full(Cout + 4, FSENT, np.float32)), be.dev(np.full(nws + 16, FSENT, np.float32))
    d = _abi.Convt16BwdWeightDesc(x=be.ptr(X), dz=be.ptr(Z), dW=be.ptr(dW), db=be.ptr(db), workspace=be.ptr(ws), workspace_floats=nws, N=N, Hi=Hi, Wi=Wi, Cin=Cin,
                                  Cout=Cout, slabs=slabs, loss_scale=scale, dtype=DT[dt])
    ok(be.lib.eegclip_convt16_bwd_weight(byref(d), be.stream))
    be.sync()
    w, b, s = be.host(dW), be.host(db), be.host(ws)
    assert (w[n:] == FSENT).all() and (b[Cout:] == FSENT).all() and (s[nws:] == FSENT).all(), "memory behind an output was written"
    assert (w[:n] != FSENT).all() and (b[:Cout] != FSENT).all(), "an element was left unwritten"
    return w[:n].reshape(Cin, Cout, 4, 4).copy(), b[:Cout].copy()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("N,Hi,Wi,Cin,Cout", CASES)
def test_bwd_weight(be, N, Hi, Wi, Cin, Cout, dt):
    rng = np.random.default_rng(7000 * N + 100 * Hi + 10 * Wi + Cin + Cout)
    x16, x = to16(rng.standard_normal((N, Hi, Wi, Cin)).astype(np.float32), dt)
    zdev, z64 = make_dz(rng, N, Hi, Wi, Cout, dt)
    x64 = x.astype(np.float64).transpose(0, 3, 1, 2)
    ref, mag = bwd_weight_ref(x64, z64), bwd_weight_ref(np.abs(x64), np.abs(z64))
    bref, bmag = z64.sum((0, 2, 3)), np.abs(z64).sum((0, 2, 3))
    X, Z = be.dev(frame_of(x16)), be.dev(zdev)
    M = N * Hi * Wi
    auto = be.lib.eegclip_convt16_bwd_weight_slabs(N, Hi, Wi, Cin, Cout)
    most = M if Cout < 16 else (M + 31) // 32
    assert 1 <= auto <= most
    if (N, Hi, Wi) == (1, 9, 15):
        assert auto > 1, "this case is here for the split-K slabs"
    for slabs, scale in sorted({(auto, 1.0), (1, 256.0), (min(3, most), 4.0), (most, 1.0)}):
        dW, db = run_weight(be, X, Z, N, Hi, Wi, Cin, Cout, dt, slabs, scale)
        assert np.isfinite(dW).all() and np.isfinite(db).all()
        bound = (M + slabs + 1) * 2.0 ** -24 * mag / scale + 1e-45
        ratio = float((np.abs(dW.astype(np.float64) - ref / scale) / bound).max())
        bratio = float((np.abs(db.astype(np.float64) - bref / scale) / ((4 * M + 2 * slabs + 1) * 2.0 ** -24 * bmag / scale)).max())
        print(f"convt16_bwd_weight {be.name} N={N} {Hi}x{Wi} {Cin}x{Cout} {dt} slabs={slabs}: worst |error| / bound dW {ratio:.3f} db {bratio:.3f} "
              f"(so far {note('weight', be, dt, max(ratio, bratio)):.3f})")
        assert ratio <= 1.0 and bratio <= 1.0
        if Hi == 1:
            assert not dW[:, :, [0, 3], :].any(), "a dead tap's gradient is not exactly 0"
        if Wi == 1:
            assert not dW[:, :, :, [0, 3]].any(), "a dead tap's gradient is not exactly 0"
        assert np.abs(dW[:, :, 1:3, 1:3]).min() > 0
        dW2, db2 = run_weight(be, X, Z, N, Hi, Wi, Cin, Cout, dt, slabs, scale)
        assert np.array_equal(dW2.view(np.uint32), dW.view(np.uint32)) and np.array_equal(db2.view(np.uint32), db.view(np.uint32)), "two runs differ"


def test_bwd_weight_rejections(be):
    N, Hi, Wi, Cin, Cout = 1, 4, 4, 128, 64
    X = be.zeros((N, Hi + 2, Wi + 2, Cin + 8), np.uint16)
    Z = be.zeros((N, 2 * Hi + 2, 2 * Wi + 2, Cout + 8), np.uint16)
    dW, db, ws = be.zeros(Cin * Cout * 16 + 8), be.zeros(Cout + 8), be.zeros(2 * Cin * Cout * 16 + 4 * Cout + 8)
    nws = be.lib.eegclip_convt16_bwd_weight_workspace_floats(N, Hi, Wi, Cin, Cout, 1)
    assert nws == Cout and be.lib.eegclip_convt16_bwd_weight_workspace_floats(N, Hi, Wi, Cin, Cout, 2) == 2 * Cin * Cout * 16 + 2 * Cout
    assert be.lib.eegclip_convt16_bwd_weight_workspace_floats(N, Hi, Wi, 96, Cout, 1) == 0 and be.lib.eegclip_convt16_bwd_weight_slabs(N, Hi, Wi, Cin, 32) == 0

    def f(**over):
        kw = dict(x=be.ptr(X), dz=be.ptr(Z), dW=be.ptr(dW), db=be.ptr(db), workspace=be.ptr(ws), workspace_floats=nws, N=N, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, slabs=1,
                  loss_scale=1.0, dtype=0)
        kw.update(over)
        return be.lib.eegclip_convt16_bwd_weight(byref(_abi.Convt16BwdWeightDesc(**kw)), be.stream)

    assert f() == 0 and f(db=None) == 0
    assert f(Cin=96) == EINVAL and f(Cout=32) == EINVAL and f(N=0) == EINVAL and f(Wi=0) == EINVAL and f(dtype=2) == EINVAL
    assert f(slabs=0) == EINVAL and f(slabs=2) == EINVAL                # the second: only one 32-pixel tile, and a workspace for one slab
    assert f(loss_scale=0.0) == EINVAL and f(loss_scale=-1.0) == EINVAL
    assert f(workspace_floats=nws - 1) == EINVAL and f(workspace=None) == EINVAL and f(x=None) == EINVAL and f(dW=None) == EINVAL
    assert f(x=be.ptr(X) + 2) == EALIGN and f(dz=be.ptr(Z) + 8) == EALIGN and f(dW=be.ptr(dW) + 4) == EALIGN and f(workspace=be.ptr(ws) + 8) == EALIGN
    assert f(db=be.ptr(db) + 2) == EALIGN
    assert be.lib.eegclip_convt16_bwd_weight(None, be.stream) == EINVAL
    be.sync()
