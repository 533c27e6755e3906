"""csrc/self_attn.hip: flash-style attention (head_dim 64, 16-bit I/O) against the fp64 oracle, on the lane emulator and on the GPU."""
import numpy as np
import pytest
import torch

from backends import be, ok  # noqa: F401
from oracle import sdxl_attn

SENTINEL = 0x7BCD                      # a finite 16-bit pattern in both dtypes; never produced by the kernel for these inputs


def _round16(a, f16):
    """float32 array -> (16-bit bit pattern as int16, the rounded values as float64)"""
    t16 = torch.tensor(np.asarray(a, np.float32)).to(torch.float16 if f16 else torch.bfloat16)
    return t16.view(torch.int16).numpy().copy(), t16.double().numpy()


def _from16(bits, f16):
    return torch.tensor(np.ascontiguousarray(bits)).view(torch.float16 if f16 else torch.bfloat16).double().numpy()


def _tol(f16):
    return 6e-3 if f16 else 2.5e-2    # the cross-attention kernel's: 16-bit probabilities and outputs


def _run(be, q, k, v, heads, f16, scale=0.125, fused=False, ldo_extra=0, extra_rows=0):
    """q (B,Tq,C), k/v (B,Tk,C) float32 -> (output values (B,Tq,C), rounded q/k/v, the raw out buffer).  fused: q lives at columns [0, C) of a
    (B,Tq,3C) buffer and k / v at [C, 2C) / [2C, 3C) of a (B,Tk,3C) one (one buffer when Tq == Tk), strides 3C."""
    B, Tq, C = q.shape
    Tk = k.shape[1]
    q16, qf = _round16(q, f16)
    k16, kf = _round16(k, f16)
    v16, vf = _round16(v, f16)
    esz = 2
    if fused:
        qb = np.zeros((B, Tq, 3 * C), np.int16)
        qb[..., :C] = q16
        kvb = qb if Tq == Tk else np.zeros((B, Tk, 3 * C), np.int16)
        kvb[..., C:2 * C], kvb[..., 2 * C:] = k16, v16
        QB = be.dev(qb)
        KVB = QB if kvb is qb else be.dev(kvb)
        bufs = (QB, KVB)
        pq, pk, pv = be.ptr(QB), be.ptr(KVB) + C * esz, be.ptr(KVB) + 2 * C * esz
        ldq = ldk = ldv = 3 * C
    else:
        Q, K, V = be.dev(q16), be.dev(k16), be.dev(v16)
        bufs = (Q, K, V)
        pq, pk, pv = be.ptr(Q), be.ptr(K), be.ptr(V)
        ldq = ldk = ldv = C
    ldo = C + ldo_extra
    OUT = be.dev(np.full((B, Tq + extra_rows, ldo), SENTINEL, np.int16)) if (ldo_extra or extra_rows) else be.zeros((B, Tq, C), np.int16)
    ok(be.lib.eegclip_self_attn_fwd(pq, ldq, pk, ldk, pv, ldv, be.ptr(OUT), ldo, B, Tq, Tk, heads, 64, float(scale), int(f16), be.stream))
    be.sync()
    del bufs
    raw = be.host(OUT)
    if ldo_extra or extra_rows:
        # the kernel indexes sample b's rows from b * Tq * ldo: view the buffer as (B * (Tq + extra_rows)) rows
        flat = raw.reshape(-1, ldo)
        got = _from16(flat[:B * Tq].reshape(B, Tq, ldo)[..., :C], f16)
    else:
        got = _from16(raw, f16)
    return got, (qf, kf, vf), raw


def _ref(qf, kf, vf, heads, scale=0.125):
    # the oracle divides the scores by sqrt(64) = 8: fold any other scale into q (fp64, exact enough)
    return sdxl_attn.cross_attention(qf * (scale * 8.0), kf, vf, heads)


def _check(got, ref, f16):
    tol = _tol(f16)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, atol=tol)
    assert np.abs(got - ref).mean() < tol / 6


@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,Tq,Tk,heads", [(1, 64, 64, 1), (2, 200, 200, 3), (1, 77, 300, 2), (1, 257, 257, 1)])
def test_self_attention_matches_oracle(be, B, Tq, Tk, heads, f16, fused):
    rng = np.random.default_rng(B * 1000 + Tq * 7 + Tk + heads + 2 * int(f16) + int(fused))
    C = heads * 64
    q, k, v = (rng.standard_normal((B, T, C)).astype(np.float32) for T in (Tq, Tk, Tk))
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16, fused=fused)
    _check(got, _ref(qf, kf, vf, heads), f16)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ["late_max", "early_max", "large_negative", "huge_scores"])
def test_online_softmax_stress(be, case, f16):
    """the running max must be rescaled correctly: maxima that only appear in the LAST key tile (+40 over every earlier score), maxima in the
    first tile that make all later tiles negligible, scores far below zero everywhere, and |scores| ~ 1e9 (inputs near the fp16 range: the
    exponent of the row maximum must stay <= 0 there, no inf)"""
    rng = np.random.default_rng({"late_max": 1, "early_max": 2, "large_negative": 3, "huge_scores": 4}[case] + 10 * int(f16))
    B, T, heads = 1, 200, 2
    C = heads * 64
    q = 0.3 * rng.standard_normal((B, T, C)).astype(np.float32)
    k = 0.3 * rng.standard_normal((B, T, C)).astype(np.float32)
    v = rng.standard_normal((B, T, C)).astype(np.float32)
    for h in range(heads):
        q[..., 64 * h] = 16.0                                          # score ~ q[0] k[0] / 8 = 2 k[0]
        if case == "late_max":
            k[:, 192:, 64 * h] = 20.0                                  # keys 192..199 = the last tile (64-key tiles): scores ~ +40
        elif case == "early_max":
            k[:, :8, 64 * h] = 20.0                                    # first tile
            k[:, 8:, 64 * h] = -5.0
        elif case == "large_negative":
            k[..., 64 * h] = -30.0 + 2.0 * rng.standard_normal((B, T)).astype(np.float32)   # scores ~ -60 +- 4
    if case == "huge_scores":
        q = 2e4 * rng.standard_normal((B, T, C)).astype(np.float32).clip(-2, 2)
        k = 2e4 * rng.standard_normal((B, T, C)).astype(np.float32).clip(-2, 2)
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16)
    _check(got, _ref(qf, kf, vf, heads), f16)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_non_default_scale(be, f16):
    rng = np.random.default_rng(7 + int(f16))
    B, Tq, Tk, heads = 2, 90, 130, 2
    C = heads * 64
    q, k, v = (rng.standard_normal((B, T, C)).astype(np.float32) * 2 for T in (Tq, Tk, Tk))
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16, scale=0.05)
    _check(got, _ref(qf, kf, vf, heads, scale=0.05), f16)
    assert np.abs(got - _ref(qf, kf, vf, heads)).max() > 5 * _tol(f16)      # (the scale is not ignored)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_writes_stay_inside_the_output_rows_and_heads(be, f16):
    """out rows >= Tq and columns outside [0, heads*64) of a wider (ldo > C), taller buffer keep their sentinel"""
    rng = np.random.default_rng(11)
    B, Tq, Tk, heads, extra_rows, ldo_extra = 2, 70, 100, 2, 9, 64
    C = heads * 64
    q, k, v = (rng.standard_normal((B, T, C)).astype(np.float32) for T in (Tq, Tk, Tk))
    got, (qf, kf, vf), raw = _run(be, q, k, v, heads, f16, ldo_extra=ldo_extra, extra_rows=extra_rows)
    _check(got, _ref(qf, kf, vf, heads), f16)
    flat = raw.reshape(-1, C + ldo_extra)
    assert (flat[:B * Tq, C:] == SENTINEL).all(), "columns beyond heads*64 were written"
    assert (flat[B * Tq:] == SENTINEL).all(), "rows beyond B*Tq were written"


def test_rejections(be):
    C, B, T, heads = 128, 1, 16, 2
    buf = be.zeros((B, T, 3 * C), np.int16)
    out = be.zeros((B, T, C), np.int16)
    p, po = be.ptr(buf), be.ptr(out)
    sup = be.lib.eegclip_self_attn_supported

    def fwd(hd=64, ld=C, ldo=C, B_=B, Tq=T, Tk=T, h=heads, q=p, scale=0.125, dtype=1):
        return be.lib.eegclip_self_attn_fwd(q, ld, p, ld, p, ld, po, ldo, B_, Tq, Tk, h, hd, scale, dtype, be.stream)

    assert sup(64, C, C, C, C) == 0 and sup(64, 3 * C, 3 * C, 3 * C, C) == 0
    for hd in (40, 128):
        assert fwd(hd=hd) < 0 and sup(hd, C, C, C, C) < 0
    assert fwd(ld=C + 4) < 0 and sup(64, C + 4, C, C, C) < 0            # stride not a multiple of 8
    assert fwd(ldo=C + 2) < 0 and sup(64, C, C, C, C + 2) < 0
    assert fwd(q=p + 2) < 0                                            # base not 16-byte aligned
    for kw in ({"B_": 0}, {"Tq": 0}, {"Tk": 0}, {"h": 0}):
        assert fwd(**kw) < 0
    assert fwd(ld=64) < 0                                              # stride shorter than heads * 64
    assert fwd(dtype=7) < 0 and fwd(scale=0.0) < 0 and fwd(scale=-0.125) < 0
    assert fwd() == 0
