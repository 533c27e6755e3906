"""csrc/self_attn.hip at head dim 80 (eegclip_attn80_fwd): flash-style attention (CLIP ViT-H/14's image tower), 16-bit I/O, against an fp64 softmax(scale q k^T) v on the 16-bit-rounded
inputs, on the lane emulator and on the GPU.

Tolerances: tests/attn_models.py's flash_model is the kernel's stated arithmetic (fp32 scores, un-normalised base-2 probabilities rounded to the I/O type, fp32
accumulation and row sum, one division, one output rounding) on the CPU; `python tests/attn_models.py` measures it against fp64 on the exact inputs of every test here
that compares with the reference.  MODEL below holds its worst max and worst mean error per group; a test's atol and mean bound are 3x those (the margin
test_kernels_vae_attn.py gives for summation order and the rescaling of the running maximum), all of them inside the 6e-3 / 2.5e-2 and a sixth of it that these tests
had before (tests/test_kernels_self_attn.py's):
  parity (N(0, 1) inputs, scale 80^-1/2: unit-variance scores, |out| < 1.6)                   atol 1.1e-3 (f16) / 7.5e-3 (bf16), mean 1.2e-4 / 9.6e-4
  late_max, early_max (8 keys share a row's weight: probabilities of 1 / 8, not of 1 / 100)  1.3e-3 / 1.4e-2, 1.9e-4 / 1.7e-3;  1.3e-3 / 1.5e-2, 2.0e-4 / 1.6e-3
  large_negative (scores spread by +- 4: single keys dominate, |out| reaches 2.7)             3.1e-3 / 2.3e-2, 2.5e-4 / 1.8e-3
  huge_scores (one-hot: the model returns v[argmax] exactly)                                  the parity bounds"""
import numpy as np
import pytest
import torch

import attn_models as am
from backends import be, ok  # noqa: F401

SENTINEL = 0x7BCD                      # a finite 16-bit pattern in both dtypes; never produced by the kernel for these inputs
NAN16 = 0x7FFF                         # a NaN in fp16 and in bf16
D = 80
SCALE = 80.0 ** -0.5


def _round16(a, f16):
    """float32 array -> (16-bit bit pattern as int16, the rounded values as float64)"""
    t16 = torch.tensor(np.asarray(a, np.float32)).to(torch.float16 if f16 else torch.bfloat16)
    return t16.view(torch.int16).numpy().copy(), t16.double().numpy()


def _from16(bits, f16):
    return torch.tensor(np.ascontiguousarray(bits)).view(torch.float16 if f16 else torch.bfloat16).double().numpy()


OLD = {True: (6e-3, 6e-3 / 6), False: (2.5e-2, 2.5e-2 / 6)}              # the (atol, bound of the mean) these tests had: tests/test_kernels_self_attn.py's
MODEL = {                                                                # worst (max, mean) error of flash_model against fp64: f16, bf16
    "parity": ((3.6e-4, 4.1e-5), (2.5e-3, 3.2e-4)),
    "late_max": ((4.2e-4, 6.3e-5), (4.6e-3, 5.7e-4)),
    "early_max": ((4.4e-4, 6.5e-5), (4.9e-3, 5.3e-4)),
    "large_negative": ((1.03e-3, 8.4e-5), (7.7e-3, 6.1e-4)),
}
MODEL["huge_scores"] = MODEL["parity"]                                   # (the model is exact there, out = v[argmax]: the parity bounds apply)


def _bounds(group, f16):
    """(atol, bound of the mean) = 3x the model's worst, at most the old bound"""
    return tuple(min(3 * m, old) for m, old in zip(MODEL[group][0 if f16 else 1], OLD[f16]))


def _ref(qf, kf, vf, heads, scale=SCALE):
    """fp64 softmax(scale q k^T) v per head of 80; q (B,Tq,C), k / v (B,Tk,C)"""
    B, Tq, C = qf.shape
    out = np.empty_like(qf)
    for h in range(heads):
        sl = slice(D * h, D * h + D)
        s = scale * np.einsum("bid,bjd->bij", qf[..., sl], kf[..., sl])
        s -= s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(axis=-1, keepdims=True)
        out[..., sl] = np.einsum("bij,bjd->bid", p, vf[..., sl])
    return out


def _check(got, ref, f16, group="parity"):
    atol, mean = _bounds(group, f16)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    print(f"attn80 max abs err {err.max():.3e} (tol {atol:.2e}), mean {err.mean():.3e} (tol {mean:.2e}), max |ref| {np.abs(ref).max():.2f}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)
    assert err.mean() < mean


def _run(be, q, k, v, heads, f16, scale=SCALE, fused=False, gutter=0, extra_rows=0):
    """q (B,Tq,C), k/v (B,Tk,C) float32 -> (output values (B,Tq,C), rounded q/k/v, the raw out buffer).  fused: q at columns [0, C) of a (B,Tq,3C) buffer,
    k / v at [C, 2C) / [2C, 3C) of a (B,Tk,3C) one (one buffer when Tq == Tk).  gutter: every operand sits in rows of C + gutter columns; the gutter of q, k, v
    holds NaN bit patterns, the gutter of out and `extra_rows` rows behind it hold SENTINEL."""
    B, Tq, C = q.shape
    Tk = k.shape[1]
    q16, qf = _round16(q, f16)
    k16, kf = _round16(k, f16)
    v16, vf = _round16(v, f16)
    if fused:
        qb = np.zeros((B, Tq, 3 * C), np.int16)
        qb[..., :C] = q16
        kvb = qb if Tq == Tk else np.zeros((B, Tk, 3 * C), np.int16)
        kvb[..., C:2 * C], kvb[..., 2 * C:] = k16, v16
        QB = be.dev(qb)
        KVB = QB if kvb is qb else be.dev(kvb)
        bufs = (QB, KVB)
        pq, pk, pv = be.ptr(QB), be.ptr(KVB) + C * 2, be.ptr(KVB) + 2 * C * 2
        ldq = ldk = ldv = 3 * C
    else:
        def pad(a16):
            buf = np.full(a16.shape[:2] + (C + gutter,), NAN16, np.int16)
            buf[..., :C] = a16
            return be.dev(buf)
        bufs = (pad(q16), pad(k16), pad(v16))
        pq, pk, pv = (be.ptr(t) for t in bufs)
        ldq = ldk = ldv = C + gutter
    ldo = C + gutter
    OUT = be.dev(np.full((B * Tq + extra_rows, ldo), SENTINEL, np.int16))
    ok(be.lib.eegclip_attn80_fwd(pq, ldq, pk, ldk, pv, ldv, be.ptr(OUT), ldo, B, Tq, Tk, heads, float(scale), int(f16), be.stream))
    be.sync()
    del bufs
    raw = be.host(OUT)
    return _from16(raw[:B * Tq].reshape(B, Tq, ldo)[..., :C], f16), (qf, kf, vf), raw


PARITY = [(1, 64, 64, 1), (2, 200, 200, 3), (1, 77, 300, 2)]


def _normal_inputs(seed, B, Tq, Tk, heads):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((B, T, heads * D)).astype(np.float32) for T in (Tq, Tk, Tk))


def _parity_inputs(B, Tq, Tk, heads, f16, fused):
    return _normal_inputs(B * 1000 + Tq * 7 + Tk + heads + 2 * int(f16) + int(fused), B, Tq, Tk, heads)


@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,Tq,Tk,heads", PARITY)
def test_attn80_matches_fp64(be, B, Tq, Tk, heads, f16, fused):
    q, k, v = _parity_inputs(B, Tq, Tk, heads, f16, fused)
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16, fused=fused)
    _check(got, _ref(qf, kf, vf, heads), f16)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_attn80_at_the_towers_token_count(be, f16):
    B, T, heads = 1, 257, 2
    q, k, v = _normal_inputs(257 + int(f16), B, T, T, heads)
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16, fused=True)
    _check(got, _ref(qf, kf, vf, heads), f16)


def _dirty_the_scratchpad(be):
    """a 64-wide launch on large NaN-free values first: on the emulator the next launch's LDS then holds them (not relied upon: the kernel must pass with
    any LDS content, this only makes a read of uninitialised LDS show up as a wrong or non-finite output here)"""
    big = be.dev(np.full((1, 64, 192), 0x7BFF, np.int16))          # fp16 65504 / a huge bf16
    out = be.zeros((1, 64, 64), np.int16)
    ok(be.lib.eegclip_self_attn_fwd(be.ptr(big), 192, be.ptr(big) + 128, 192, be.ptr(big) + 256, 192, be.ptr(out), 64, 1, 64, 64, 1, 64, 1e-6, 1, be.stream))
    be.sync()


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_pad_columns_never_come_from_memory(be, f16):
    """columns 80..95 of the third k-step do not exist: behind the last head of q, k, v lie 16 gutter columns of NaN (ld = C + 16), `out` has a sentinel gutter
    and sentinel rows behind it.  The output must be finite and right, the gutters and the rows untouched."""
    _dirty_the_scratchpad(be)
    B, Tq, Tk, heads, extra_rows = 2, 70, 100, 2, 9
    C = heads * D
    q, k, v = _normal_inputs(80 + int(f16), B, Tq, Tk, heads)
    got, (qf, kf, vf), raw = _run(be, q, k, v, heads, f16, gutter=16, extra_rows=extra_rows)
    _check(got, _ref(qf, kf, vf, heads), f16)
    assert (raw[:B * Tq, C:] == SENTINEL).all(), "columns beyond heads * 80 were written"
    assert (raw[B * Tq:] == SENTINEL).all(), "rows beyond B * Tq were written"


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ["late_max", "early_max", "large_negative", "huge_scores"])
def test_online_softmax_stress(be, case, f16):
    """tests/test_kernels_self_attn.py's stress cases at head dim 80: maxima that only appear in the last key tile, maxima in the first tile, scores far
    below zero everywhere, |scores| ~ 1e9"""
    q, k, v, heads = _stress_inputs(case, f16)
    got, (qf, kf, vf), _ = _run(be, q, k, v, heads, f16)
    _check(got, _ref(qf, kf, vf, heads), f16, case)


def _stress_inputs(case, f16):
    rng = np.random.default_rng({"late_max": 1, "early_max": 2, "large_negative": 3, "huge_scores": 4}[case] + 10 * int(f16))
    B, T, heads = 1, 200, 2
    C = heads * D
    q = 0.3 * rng.standard_normal((B, T, C)).astype(np.float32)
    k = 0.3 * rng.standard_normal((B, T, C)).astype(np.float32)
    v = rng.standard_normal((B, T, C)).astype(np.float32)
    for h in range(heads):
        q[..., D * h] = 16.0                                           # score ~ q[0] k[0] * 80^-1/2 = 1.8 k[0]
        if case == "late_max":
            k[:, 192:, D * h] = 20.0                                   # keys 192..199 = the last tile (64-key tiles): scores ~ +36
        elif case == "early_max":
            k[:, :8, D * h] = 20.0                                     # first tile
            k[:, 8:, D * h] = -5.0
        elif case == "large_negative":
            k[..., D * h] = -30.0 + 2.0 * rng.standard_normal((B, T)).astype(np.float32)   # scores ~ -54 +- 4
    if case == "huge_scores":
        q = 2e4 * rng.standard_normal((B, T, C)).astype(np.float32).clip(-2, 2)
        k = 2e4 * rng.standard_normal((B, T, C)).astype(np.float32).clip(-2, 2)
    return q, k, v, heads


def test_two_runs_are_bit_identical(be):
    rng = np.random.default_rng(5)
    B, Tq, Tk, heads = 2, 130, 200, 2
    q, k, v = (rng.standard_normal((B, T, heads * D)).astype(np.float32) for T in (Tq, Tk, Tk))
    a = _run(be, q, k, v, heads, True)[2]
    b = _run(be, q, k, v, heads, True)[2]
    assert np.array_equal(a, b)


def test_rejections(be):
    heads, B, T = 2, 1, 16
    C = heads * D
    buf = be.zeros((B, T, 3 * C), np.int16)
    out = be.zeros((B, T, C), np.int16)
    p, po = be.ptr(buf), be.ptr(out)
    sup = be.lib.eegclip_attn80_supported

    def fwd(ld=C, ldo=C, B_=B, Tq=T, Tk=T, h=heads, q=p, scale=SCALE, dtype=1):
        return be.lib.eegclip_attn80_fwd(q, ld, p, ld, p, ld, po, ldo, B_, Tq, Tk, h, scale, dtype, be.stream)

    EINVAL, EALIGN = -1, -2                                            # include/eegclip.h; the 64-wide kernel's codes, in its order
    assert sup(C, C, C, C) == 0 and sup(3 * C, 3 * C, 3 * C, C) == 0
    assert fwd(ld=C + 4) == EALIGN and sup(C + 4, C, C, C) == EALIGN   # stride not a multiple of 8
    assert fwd(ldo=C + 2) == EALIGN and sup(C, C, C, C + 2) == EALIGN
    assert sup(72, C, C, C) == EINVAL and sup(76, C, C, C) == EINVAL   # stride below one head: EINVAL before the alignment (76 is no multiple of 8)
    assert fwd(ld=80) == EINVAL and fwd(ldo=80) == EINVAL              # stride below heads * 80
    assert fwd(q=p + 2) == EALIGN                                      # base not 16-byte aligned
    for kw in ({"B_": 0}, {"Tq": 0}, {"Tk": 0}, {"h": 0}):
        assert fwd(**kw) == EINVAL
    assert fwd(dtype=7) == EINVAL and fwd(scale=0.0) == EINVAL and fwd(scale=-0.1) == EINVAL
    assert fwd(ld=C + 4, h=0) == EALIGN                                # the stride checks come first ...
    assert fwd(q=p + 2, dtype=7) == EINVAL and fwd(q=p + 2, B_=0) == EINVAL      # ... and every EINVAL of the arguments before the base alignment
    same = be.lib.eegclip_self_attn_fwd                                # the 64-wide entry point answers the same cases alike
    assert same(p + 2, 128, p, 128, p, 128, po, 128, B, T, T, 2, 64, SCALE, 7, be.stream) == EINVAL
    assert same(p, 132, p, 128, p, 128, po, 128, B, T, T, 0, 64, SCALE, 1, be.stream) == EALIGN
    assert fwd() == 0
    # the 64-wide entry points keep rejecting every other head dim
    assert be.lib.eegclip_self_attn_fwd(p, C, p, C, p, C, po, C, B, T, T, heads, 80, SCALE, 1, be.stream) < 0


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("Tk", [63, 64, 65, 128, 200])
def test_every_key_counted_exactly_once(be, Tk, f16):
    """q = 0 makes the attention uniform; v[j] = Tk * onehot((j + h) mod 80) turns the output into the integer count of keys per column: a dropped,
    duplicated or mis-masked key moves an entry by 1.0 (or, a padding key let in, scales a row by Tk / (Tk + n)).  Tk <= 256 is exact in bf16, and the
    un-normalised probabilities are all exactly 1.  Tq = 70 is a second workgroup with one partial query tile."""
    B, heads, Tq = 1, 2, 70
    rng = np.random.default_rng(Tk + int(f16))
    q = np.zeros((B, Tq, heads * D), np.float32)
    k = rng.standard_normal((B, Tk, heads * D)).astype(np.float32)
    v, count = am.count_values(B, Tk, heads, D)
    got, _, _ = _run(be, q, k, v, heads, f16, fused=Tk == 65)
    print(f"max error {np.abs(got - count).max():.3e}")
    np.testing.assert_allclose(got, np.broadcast_to(count, got.shape), rtol=0, atol=0.05)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,heads,Tq,Tk", [(1, 2, 70, 65), (2, 3, 130, 159), (1, 2, 70, 300)])
def test_each_query_returns_its_own_value_row(be, B, heads, Tq, Tk, f16):
    """q[i] = k[target(i)], target(i) = (5 i + h) mod Tk, scale 1 / 8, with keys that score 32 below the target against every other query: +-16 unit vectors
    for Tk <= 160, a two-hot code (16 (e_a + e_b): 64 against itself, 32 or 0 against another) beyond.  The attention is one-hot up to e^-32 tails and the
    output is v[target], small integers that differ by key, column, head and sample: a k-slot permutation between P and V^T, a wrong key tile (Tk = 300:
    five of them, the double buffer wraps), query tile, head or workgroup offset returns ANOTHER row (an error of order 10).  The codes use columns 64 .. 79
    too, the third k-step's half that exists."""
    k = am.onehot_keys(B, Tk, heads, D) if Tk <= 2 * D else am.twohot_keys(B, Tk, heads, D)
    v = am.int_values(B, Tk, heads, D)
    tgt = am.targets(Tq, Tk, heads)
    want = am.gather_rows(v, tgt, heads).astype(np.float64)
    got, (qf, kf, vf), _ = _run(be, am.gather_rows(k, tgt, heads), k, v, heads, f16, scale=0.125, fused=Tk == 159)
    np.testing.assert_allclose(_ref(qf, kf, vf, heads, scale=0.125), want, rtol=0, atol=1e-9, err_msg="the construction itself is no longer one-hot")
    print(f"max error {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def _model_case(inputs, heads, f16):
    def make():
        qf, kf, vf = (am.round16(a, f16) for a in inputs()[:3])
        return am.flash_model(qf, kf, vf, heads, SCALE, f16), _ref(qf, kf, vf, heads)
    return make


# what `python tests/attn_models.py` measures the model on: the exact inputs of every test here that goes through _check
MODEL_CASES = {
    "parity": [(f"{s} fused={fu}", f16, _model_case(lambda s=s, f16=f16, fu=fu: _parity_inputs(*s, f16, fu), s[3], f16))
               for s in PARITY for f16 in (True, False) for fu in (False, True)]
              + [("towers", f16, _model_case(lambda f16=f16: _normal_inputs(257 + int(f16), 1, 257, 257, 2), 2, f16)) for f16 in (True, False)]
              + [("gutter", f16, _model_case(lambda f16=f16: _normal_inputs(80 + int(f16), 2, 70, 100, 2), 2, f16)) for f16 in (True, False)],
    **{case: [(case, f16, _model_case(lambda case=case, f16=f16: _stress_inputs(case, f16), 2, f16)) for f16 in (True, False)]
       for case in ("late_max", "early_max", "large_negative", "huge_scores")},
}
