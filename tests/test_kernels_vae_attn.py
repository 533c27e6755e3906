"""csrc/vae_attn.hip: single-head flash attention over wide heads (head_dim 128 .. 512, 16-bit I/O) against an fp64 numpy reference on the
16-bit-rounded inputs, on the lane emulator and on the GPU.

Tolerances: a CPU model of the kernel's stated arithmetic (fp32 scores, 16-bit probabilities, fp32 accumulation, one output rounding) on N(0, 1)
inputs at these shapes has a worst max error of 3.0e-4 (f16) / 2.4e-3 (bf16) and a mean error of 3.9e-5 / 3.1e-4; atol = 1e-3 / 8e-3 and
mean < atol / 6 leave about 3x for summation order and the rescaling of the running maximum."""
import math

import numpy as np
import pytest
import torch

from backends import be, ok  # noqa: F401

SENTINEL = 0x7BCD                      # a finite 16-bit pattern in both dtypes; never produced by the kernel for these inputs
DTYPES = pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])


def _round16(a, f16):
    """float32 array -> (16-bit bit pattern as int16, the rounded values as float64)"""
    t16 = torch.tensor(np.asarray(a, np.float32)).to(torch.float16 if f16 else torch.bfloat16)
    return t16.view(torch.int16).numpy().copy(), t16.double().numpy()


def _from16(bits, f16):
    return torch.tensor(np.ascontiguousarray(bits)).view(torch.float16 if f16 else torch.bfloat16).double().numpy()


def _tol(f16):
    return 1e-3 if f16 else 8e-3


def _run(be, q, k, v, f16, scale=None, packed=False, ldo_extra=0, extra_rows=0):
    """q, k, v (B, T, D) float32 -> (output values (B, T, D), rounded q / k / v, the raw out buffer as (rows, ldo)).  packed: q, k, v are the
    column blocks [0, D), [D, 2D), [2D, 3D) of one (B * T, 3D) buffer, strides 3D."""
    B, T, D = q.shape
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    q16, qf = _round16(q, f16)
    k16, kf = _round16(k, f16)
    v16, vf = _round16(v, f16)
    if packed:
        buf = np.zeros((B * T, 3 * D), np.int16)
        buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:] = q16.reshape(-1, D), k16.reshape(-1, D), v16.reshape(-1, D)
        bufs = (be.dev(buf),)
        pq, pk, pv = be.ptr(bufs[0]), be.ptr(bufs[0]) + 2 * D, be.ptr(bufs[0]) + 4 * D
        ldq = ldk = ldv = 3 * D
    else:
        bufs = (be.dev(q16), be.dev(k16), be.dev(v16))
        pq, pk, pv = (be.ptr(t) for t in bufs)
        ldq = ldk = ldv = D
    ldo = D + ldo_extra
    OUT = be.dev(np.full((B * T + extra_rows, ldo), SENTINEL, np.int16))
    ok(be.lib.eegclip_vae_attn_fwd(pq, ldq, pk, ldk, pv, ldv, be.ptr(OUT), ldo, B, T, D, float(scale), int(f16), be.stream))
    be.sync()
    del bufs
    raw = be.host(OUT)
    return _from16(raw[:B * T, :D].reshape(B, T, D), f16), (qf, kf, vf), raw


def _ref(qf, kf, vf, scale=None):
    s = np.einsum("bid,bjd->bij", qf, kf) * (1.0 / math.sqrt(qf.shape[-1]) if scale is None else scale)
    p = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("bij,bjd->bid", p / p.sum(-1, keepdims=True), vf)


def _check(got, ref, f16):
    tol = _tol(f16)
    err = np.abs(got - ref)
    print(f"max error {err.max():.3e} (atol {tol:.0e}), mean error {err.mean():.3e} (bound {tol / 6:.2e})")
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=tol)
    assert err.mean() < tol / 6


@DTYPES
@pytest.mark.parametrize("B,T,D", [(1, 16, 128), (2, 234, 128), (1, 234, 512), (2, 77, 512), (1, 130, 384), (1, 257, 256)])
def test_matches_fp64_reference(be, B, T, D, f16):
    """less than one tile; T = 234 leaves a remainder against 16, 32 and 64 (a partial last key tile and a partial last query tile); every head_dim"""
    rng = np.random.default_rng(B * 1000 + T * 7 + D + int(f16))
    q, k, v = (rng.standard_normal((B, T, D)).astype(np.float32) for _ in range(3))
    got, (qf, kf, vf), _ = _run(be, q, k, v, f16)
    _check(got, _ref(qf, kf, vf), f16)


@DTYPES
@pytest.mark.parametrize("D", [128, 512])
def test_every_key_counted_exactly_once(be, D, f16):
    """q = 0 makes the attention uniform; v[j] = T * onehot(j mod D) turns the output into the integer count of keys per column (1 or 2 at
    D = 128, 0 or 1 at D = 512), so a dropped, duplicated or mis-masked key moves an entry by 1.0 (on N(0, 1) inputs: by ~4e-3, inside the
    tolerance).  T = 234 is exact in bf16; 1 / 234 rounded to bf16 costs at most 0.4 %."""
    B, T = 1, 234
    rng = np.random.default_rng(D + int(f16))
    q = np.zeros((B, T, D), np.float32)
    k = rng.standard_normal((B, T, D)).astype(np.float32)
    v = np.zeros((B, T, D), np.float32)
    v[0, np.arange(T), np.arange(T) % D] = float(T)
    got, _, _ = _run(be, q, k, v, f16)
    count = np.bincount(np.arange(T) % D, minlength=D).astype(np.float64)
    np.testing.assert_allclose(got, np.broadcast_to(count, got.shape), rtol=0, atol=0.05)


@DTYPES
@pytest.mark.parametrize("case", ["late_max", "early_max", "large_negative", "huge_scores"])
def test_online_softmax_stress(be, case, f16):
    """the cases of test_kernels_self_attn.py at head_dim 512: the row maximum only in the LAST 8 keys (+40 over every earlier score), the maximum in
    the first 8 keys, scores near -60 everywhere, and |scores| ~ 1e9 (inputs near the fp16 range: no inf, no NaN).  The scores near -60 spread by
    +- 1 like those of the N(0, 1) parity inputs the tolerance was derived on: a wider spread makes the softmax pick single keys, |out| reaches
    2 and the final bf16 rounding alone (half an ulp of [2, 4) is 7.8e-3) uses up the tolerance whatever the kernel does."""
    rng = np.random.default_rng({"late_max": 1, "early_max": 2, "large_negative": 3, "huge_scores": 4}[case] + 10 * int(f16))
    B, T, D = 1, 200, 512
    q = 0.3 * rng.standard_normal((B, T, D)).astype(np.float32)
    k = 0.3 * rng.standard_normal((B, T, D)).astype(np.float32)
    v = rng.standard_normal((B, T, D)).astype(np.float32)
    q[..., 0] = 2.0 * math.sqrt(D)                                     # score ~ q[0] k[0] / sqrt(D) = 2 k[0]   (45.25: exact in bf16)
    if case == "late_max":
        k[:, 192:, 0] = 20.0                                           # keys 192 .. 199, the last tile: scores ~ +40
    elif case == "early_max":
        k[:, :8, 0] = 20.0
        k[:, 8:, 0] = -5.0
    elif case == "large_negative":
        k[..., 0] = -30.0 + 0.5 * rng.standard_normal((B, T)).astype(np.float32)       # scores ~ -60 +- 1
    if case == "huge_scores":
        q = 2e4 * rng.standard_normal((B, T, D)).astype(np.float32).clip(-2, 2)
        k = 2e4 * rng.standard_normal((B, T, D)).astype(np.float32).clip(-2, 2)
    got, (qf, kf, vf), _ = _run(be, q, k, v, f16)
    _check(got, _ref(qf, kf, vf), f16)


@DTYPES
def test_non_default_scale(be, f16):
    rng = np.random.default_rng(7 + int(f16))
    B, T, D = 2, 90, 256
    q, k, v = (rng.standard_normal((B, T, D)).astype(np.float32) for _ in range(3))
    got, (qf, kf, vf), _ = _run(be, q, k, v, f16, scale=0.02)
    _check(got, _ref(qf, kf, vf, scale=0.02), f16)
    assert np.abs(got - _ref(qf, kf, vf)).max() > 5 * _tol(f16)           # (the scale is not ignored)


@DTYPES
def test_writes_stay_inside_the_output_rows_and_columns(be, f16):
    """out rows >= B * T and columns >= D of a wider (ldo = D + 64), taller (9 more rows) buffer keep their sentinel"""
    rng = np.random.default_rng(11)
    B, T, D = 2, 70, 128
    q, k, v = (rng.standard_normal((B, T, D)).astype(np.float32) for _ in range(3))
    got, (qf, kf, vf), raw = _run(be, q, k, v, f16, ldo_extra=64, extra_rows=9)
    _check(got, _ref(qf, kf, vf), f16)
    assert (raw[:B * T, D:] == SENTINEL).all(), "columns beyond head_dim were written"
    assert (raw[B * T:] == SENTINEL).all(), "rows beyond B * T were written"


@DTYPES
@pytest.mark.parametrize("D", [128, 512])
def test_strided_inputs(be, D, f16):
    """q, k, v as column blocks of one (B * T, 3 D) buffer, consumed in place"""
    rng = np.random.default_rng(13 + D)
    B, T = 2, 77
    q, k, v = (rng.standard_normal((B, T, D)).astype(np.float32) for _ in range(3))
    got, (qf, kf, vf), _ = _run(be, q, k, v, f16, packed=True)
    _check(got, _ref(qf, kf, vf), f16)


def test_rejections(be):
    D, B, T = 128, 1, 16
    buf = be.zeros((B * T, 3 * D), np.int16)
    out = be.zeros((B * T, D), np.int16)
    p, po = be.ptr(buf), be.ptr(out)
    sup = be.lib.eegclip_vae_attn_supported

    def fwd(hd=D, ld=3 * D, ldo=D, B_=B, T_=T, q=p, scale=0.125, dtype=1):
        return be.lib.eegclip_vae_attn_fwd(q, ld, p, ld, p, ld, po, ldo, B_, T_, hd, scale, dtype, be.stream)

    assert sup(D, D, D, D, D) == 0 and sup(512, 1536, 1536, 1536, 512) == 0
    for hd in (64, 640, 100):
        assert fwd(hd=hd, ld=1920, ldo=640) < 0 and sup(hd, 1920, 1920, 1920, 640) < 0
    assert fwd(ld=3 * D + 4) < 0 and sup(D, 3 * D + 4, 3 * D, 3 * D, D) < 0      # stride not a multiple of 8
    assert fwd(ldo=D + 2) < 0 and sup(D, D, D, D, D + 2) < 0
    assert fwd(ld=D - 8) < 0 and sup(D, D - 8, D, D, D) < 0                      # stride shorter than head_dim
    assert fwd(ldo=D - 8) < 0 and sup(D, D, D, D, D - 8) < 0
    assert fwd(q=p + 2) < 0                                                      # base not 16-byte aligned
    for kw in ({"B_": 0}, {"T_": 0}, {"B_": -1}, {"T_": -3}, {"scale": 0.0}, {"scale": -0.125}, {"scale": float("inf")}, {"dtype": 7}):
        assert fwd(**kw) < 0, kw
    assert fwd() == 0
    be.sync()
