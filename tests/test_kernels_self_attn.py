"""csrc/self_attn.hip: flash-style attention (head_dim 64, 16-bit I/O) against the fp64 oracle, on the lane emulator and on the GPU.

Tolerances: tests/attn_models.py's flash_model is the kernel's stated arithmetic (fp32 scores, un-normalised base-2 probabilities rounded to the I/O type, fp32
accumulation and row sum, one division, one output rounding) on the CPU; `python tests/attn_models.py` measures it against fp64 on the exact inputs of every
test here that compares with the oracle.  MODEL below holds its worst max and worst mean error per group; a test's atol and mean bound are 3x those (the
margin test_kernels_vae_attn.py gives for summation order and the rescaling of the running maximum), and never more than the 6e-3 / 2.5e-2 and a sixth of it
that these tests had before (the cross-attention kernel's):
  parity (N(0, 1) inputs at scale 1 / 8: the 64- and the 128-query form, the sentinel test)    atol 2.3e-3 (f16) / 1.98e-2 (bf16), mean 1.2e-4 / 9.9e-4
  late_max, early_max (8 keys share a row's weight: probabilities of 1 / 8, not of 1 / 100)   1.8e-3 / 1.3e-2, 2.1e-4 / 1.65e-3;  1.6e-3 / 1.5e-2, 2.0e-4 / 1.6e-3
  large_negative (scores spread by +- 4: single keys dominate, |out| reaches 2.9)              1.9e-3 / 2.4e-2, 2.5e-4 / 3.2e-3
  non_default_scale (v is 2 N(0, 1), |out| reaches 4.9; bf16: 3x the model's max is 4.3e-2, the old 2.5e-2 stays)   3.2e-3 / 2.5e-2, 2.7e-4 / 2.1e-3
  huge_scores (one-hot: the model returns v[argmax] exactly)                                   the parity bounds"""
import numpy as np
import pytest
import torch

import attn_models as am
from backends import be, ok  # noqa: F401
from oracle import sdxl_attn

SENTINEL = 0x7BCD                      # a finite 16-bit pattern in both dtypes; never produced by the kernel for these inputs


def _round16(a, f16):
    """float32 array -> (16-bit bit pattern as int16, the rounded values as float64)"""
    t16 = torch.tensor(np.asarray(a, np.float32)).to(torch.float16 if f16 else torch.bfloat16)
    return t16.view(torch.int16).numpy().copy(), t16.double().numpy()


def _from16(bits, f16):
    return torch.tensor(np.ascontiguousarray(bits)).view(torch.float16 if f16 else torch.bfloat16).double().numpy()


OLD = {True: (6e-3, 6e-3 / 6), False: (2.5e-2, 2.5e-2 / 6)}              # the (atol, bound of the mean) these tests had: the cross-attention kernel's
MODEL = {                                                                # worst (max, mean) error of flash_model against fp64: f16, bf16
    "parity": ((7.6e-4, 3.9e-5), (6.6e-3, 3.3e-4)),
    "late_max": ((6.1e-4, 7.1e-5), (4.4e-3, 5.5e-4)),
    "early_max": ((5.2e-4, 6.5e-5), (5.1e-3, 5.4e-4)),
    "large_negative": ((6.4e-4, 8.4e-5), (7.9e-3, 1.08e-3)),
    "non_default_scale": ((1.06e-3, 8.9e-5), (1.43e-2, 6.9e-4)),
}
MODEL["huge_scores"] = MODEL["parity"]                                   # (the model is exact there, out = v[argmax]: the parity bounds apply)


def _bounds(group, f16):
    """(atol, bound of the mean) = 3x the model's worst, at most the old bound"""
    return tuple(min(3 * m, old) for m, old in zip(MODEL[group][0 if f16 else 1], OLD[f16]))


def _tol(f16):
    """the atol every test here had before: tests/test_kernels_clip_text.py (the causal forms) imports it and keeps it"""
    return OLD[f16][0]


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


def _check(got, ref, f16, group="parity"):
    atol, mean = _bounds(group, f16)
    err = np.abs(got - ref)
    print(f"max error {err.max():.3e} (atol {atol:.2e}), mean error {err.mean():.3e} (bound {mean:.2e}), max |ref| {np.abs(ref).max():.2f}")
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)
    assert err.mean() < mean


PARITY = [(1, 64, 64, 1), (2, 200, 200, 3), (1, 77, 300, 2), (1, 257, 257, 1)]


def _parity_inputs(B, Tq, Tk, heads, f16, fused):
    rng = np.random.default_rng(B * 1000 + Tq * 7 + Tk + heads + 2 * int(f16) + int(fused))
    return tuple(rng.standard_normal((B, T, heads * 64)).astype(np.float32) for T in (Tq, Tk, Tk))


@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,Tq,Tk,heads", PARITY)
def test_self_attention_matches_oracle(be, B, Tq, Tk, heads, f16, fused):
    q, k, v = _parity_inputs(B, Tq, Tk, heads, f16, fused)
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16, fused=fused)
    _check(got, _ref(qf, kf, vf, heads), f16)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ["late_max", "early_max", "large_negative", "huge_scores"])
def test_online_softmax_stress(be, case, f16):
    """the running max must be rescaled correctly: maxima that only appear in the LAST key tile (+40 over every earlier score), maxima in the
    first tile that make all later tiles negligible, scores far below zero everywhere, and |scores| ~ 1e9 (inputs near the fp16 range: the
    exponent of the row maximum must stay <= 0 there, no inf)"""
    q, k, v, heads = _stress_inputs(case, f16)
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16)
    _check(got, _ref(qf, kf, vf, heads), f16, case)


def _stress_inputs(case, f16):
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
    return q, k, v, heads


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_non_default_scale(be, f16):
    q, k, v, heads = _scale_inputs(f16)
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16, scale=0.05)
    _check(got, _ref(qf, kf, vf, heads, scale=0.05), f16, "non_default_scale")
    assert np.abs(got - _ref(qf, kf, vf, heads)).max() > 5 * OLD[f16][0]      # (the scale is not ignored)


def _scale_inputs(f16):
    rng = np.random.default_rng(7 + int(f16))
    B, Tq, Tk, heads = 2, 90, 130, 2
    return tuple(rng.standard_normal((B, T, heads * 64)).astype(np.float32) * 2 for T in (Tq, Tk, Tk)) + (heads,)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_writes_stay_inside_the_output_rows_and_heads(be, f16):
    """out rows >= Tq and columns outside [0, heads*64) of a wider (ldo > C), taller buffer keep their sentinel"""
    B, Tq, Tk, heads, extra_rows, ldo_extra = 2, 70, 100, 2, 9, 64
    C = heads * 64
    q, k, v = _rows_inputs()
    got, (qf, kf, vf), raw = _run(be, q, k, v, heads, f16, ldo_extra=ldo_extra, extra_rows=extra_rows)
    _check(got, _ref(qf, kf, vf, heads), f16)
    flat = raw.reshape(-1, C + ldo_extra)
    assert (flat[:B * Tq, C:] == SENTINEL).all(), "columns beyond heads*64 were written"
    assert (flat[B * Tq:] == SENTINEL).all(), "rows beyond B*Tq were written"


def _rows_inputs():
    rng = np.random.default_rng(11)
    return tuple(rng.standard_normal((2, T, 128)).astype(np.float32) for T in (70, 100, 100))


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


# ---- the 128-query form (two query tiles per wave): sa_forward takes it when B * heads * ceil(Tq / 128) >= 512 -------------------------------------------
# (4, 64, 200, 77): the second workgroup has one full and one 8-row query tile per wave pair; two key tiles, the last partial.
# (8, 32, 150, 128): the second workgroup's second query tile lies wholly beyond Tq; two full key tiles.
WIDE = [(4, 64, 200, 77), (8, 32, 150, 128)]
WIDE_PARAMS = [pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"]),
               pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"]),
               pytest.mark.parametrize("B,heads,Tq,Tk", WIDE)]


def _wide(fn):
    for mark in WIDE_PARAMS:
        fn = mark(fn)
    return fn


def _wide_inputs(B, heads, Tq, Tk, f16, fused):
    rng = np.random.default_rng(B * 1000 + Tq * 7 + Tk + heads + 2 * int(f16) + int(fused))
    return tuple(rng.standard_normal((B, T, heads * 64)).astype(np.float32) for T in (Tq, Tk, Tk))


@_wide
def test_wide_form_matches_oracle_and_stays_inside_its_rows(be, B, heads, Tq, Tk, f16, fused):
    """N(0, 1) parity of self_attn_kernel<.., QT = 2, CAUSAL = false, 64>, into a wider (ldo = C + 64), taller (9 more rows) sentinel-filled buffer"""
    assert B * heads * ((Tq + 127) // 128) >= 512
    C = heads * 64
    q, k, v = _wide_inputs(B, heads, Tq, Tk, f16, fused)
    got, (qf, kf, vf), raw = _run(be, q, k, v, heads, f16, fused=fused, ldo_extra=64, extra_rows=9)
    _check(got, _ref(qf, kf, vf, heads), f16)
    flat = raw.reshape(-1, C + 64)
    assert (flat[:B * Tq, C:] == SENTINEL).all(), "columns beyond heads*64 were written"
    assert (flat[B * Tq:] == SENTINEL).all(), "rows beyond B*Tq were written"


def _count_test(be, B, heads, Tq, Tk, f16, fused):
    """q = 0 makes the attention uniform; v[j] = Tk * onehot((j + h) mod 64) turns the output into the integer count of keys per column: a dropped,
    duplicated or mis-masked key moves an entry by 1.0 (or, a padding key let in, scales a row by Tk / (Tk + n)).  Tk <= 256 is exact in bf16, and the
    un-normalised probabilities are all exactly 1."""
    assert Tk <= 256
    rng = np.random.default_rng(Tk + int(f16))
    C = heads * 64
    q = np.zeros((B, Tq, C), np.float32)
    k = rng.standard_normal((B, Tk, C)).astype(np.float32)
    v, count = am.count_values(B, Tk, heads, 64)
    got, _, _ = _run(be, q, k, v, heads, f16, fused=fused)
    print(f"max error {np.abs(got - count).max():.3e}")
    np.testing.assert_allclose(got, np.broadcast_to(count, got.shape), rtol=0, atol=0.05)


def _onehot_test(be, B, heads, Tq, Tk, f16, fused):
    """q[i] = k[target(i)], target(i) = (5 i + h) mod Tk, with keys that score 32 below the target against every other query: +-16 unit vectors for
    Tk <= 128, a two-hot code (16 (e_a + e_b): 64 against itself, 32 or 0 against another) beyond.  The attention is one-hot up to e^-32 tails and the
    output is v[target], small integers that differ by key, column, head and sample: a k-slot permutation between P and V^T, a wrong key tile (Tk = 300:
    five of them, the double buffer wraps), query tile, head or workgroup offset returns ANOTHER row (an error of order 10)."""
    k = am.onehot_keys(B, Tk, heads, 64) if Tk <= 128 else am.twohot_keys(B, Tk, heads, 64)
    v = am.int_values(B, Tk, heads, 64)
    tgt = am.targets(Tq, Tk, heads)
    want = am.gather_rows(v, tgt, heads).astype(np.float64)
    got, (qf, kf, vf), _ = _run(be, am.gather_rows(k, tgt, heads), k, v, heads, f16, fused=fused)
    np.testing.assert_allclose(_ref(qf, kf, vf, heads), want, rtol=0, atol=1e-9, err_msg="the construction itself is no longer one-hot")
    print(f"max error {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


@_wide
def test_wide_form_counts_every_key_exactly_once(be, B, heads, Tq, Tk, f16, fused):
    assert B * heads * ((Tq + 127) // 128) >= 512
    _count_test(be, B, heads, Tq, Tk, f16, fused)


@_wide
def test_wide_form_returns_each_querys_own_value_row(be, B, heads, Tq, Tk, f16, fused):
    assert B * heads * ((Tq + 127) // 128) >= 512
    _onehot_test(be, B, heads, Tq, Tk, f16, fused)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("Tk", [63, 64, 65, 128, 200])
def test_every_key_counted_exactly_once(be, Tk, f16):
    """the 64-query form; Tq = 70 is a second workgroup with one partial query tile"""
    _count_test(be, 1, 2, 70, Tk, f16, fused=Tk == 65)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,heads,Tq,Tk", [(1, 2, 70, 65), (1, 2, 130, 128), (2, 3, 70, 300)])
def test_each_query_returns_its_own_value_row(be, B, heads, Tq, Tk, f16):
    """the 64-query form"""
    _onehot_test(be, B, heads, Tq, Tk, f16, fused=Tk == 128)


def _model_case(inputs, scale, f16):
    def make():
        *qkv, heads = inputs()
        qf, kf, vf = (am.round16(a, f16) for a in qkv)
        return am.flash_model(qf, kf, vf, heads, scale, f16), _ref(qf, kf, vf, heads, scale)
    return make


# what `python tests/attn_models.py` measures the model on: the exact inputs of every test here that goes through _check
MODEL_CASES = {
    "parity": [(f"{s} fused={fu}", f16, _model_case(lambda s=s, f16=f16, fu=fu: _parity_inputs(*s, f16, fu) + (s[3],), 0.125, f16))
               for s in PARITY for f16 in (True, False) for fu in (False, True)]
              + [(f"wide {s} fused={fu}", f16, _model_case(lambda s=s, f16=f16, fu=fu: _wide_inputs(*s, f16, fu) + (s[1],), 0.125, f16))
                 for s in WIDE for f16 in (True, False) for fu in (False, True)]
              + [("rows", f16, _model_case(lambda: _rows_inputs() + (2,), 0.125, f16)) for f16 in (True, False)],
    **{case: [(case, f16, _model_case(lambda case=case, f16=f16: _stress_inputs(case, f16), 0.125, f16)) for f16 in (True, False)]
       for case in ("late_max", "early_max", "large_negative", "huge_scores")},
    "non_default_scale": [("scale", f16, _model_case(lambda f16=f16: _scale_inputs(f16), 0.05, f16)) for f16 in (True, False)],
}
