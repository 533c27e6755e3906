"""The caption decoder's kernels through the C ABI on both backends, against numpy fp64 on the rounded inputs: the prefix-causal form of csrc/self_attn.hip and
csrc/caption.hip (decode attention, the skinny-M GEMM).

Bounds, from the arithmetic (u = half an ulp of the 16-bit format relative to 1: 2^-11 for fp16, 2^-8 for bf16):
  * attention: o = sum_j p_j v_j / sum_j e_j with e_j = exp2(..) <= 1 in fp32, the row maximum's e = 1 (so the denominator is >= 1), p_j = e_j rounded to
    16 bit before P V (relative error <= u; below the fp16 normal range an absolute 2^-25 per key), fp32 accumulation, one division and one rounding of the
    result.  |o| <= max|v|, so:  numerator error <= u sum_j e_j |v_j| <= u max|v| (sum e_j), i.e. u max|v| after the division; the final rounding adds
    u |o| <= u max|v|.  What is left is fp32: the 64-term score dot product (<= 64 * 2^-24 * sum|q_i k_i| / 8, ~1e-5 here, the same relative change of e_j),
    v_exp_f32 (1 ulp), the accumulation over <= 300 keys (300 * 2^-24) and the subnormal probabilities (300 * 2^-25 * max|v|): together < 2e-4 for these
    inputs.   |error| <= 2 u max|v| + 2e-4.   The decode kernel keeps its probabilities in fp32 and is held to the same bound.
  * skinny GEMM: every product is exact in fp32 (two 16-bit factors), the sum of K products plus bias plus residual is accumulated in fp32 in some order:
    |error| <= (K + 2) 2^-24 (sum_k |a_k w_k| + |bias| + |r|) for any order; the 16-bit output adds one rounding, u |result| (plus the smallest subnormal).
"""
import numpy as np
import pytest

from backends import be, ok  # noqa: F401
from test_kernels_gemm16 import DT, from16, to16

SENT = 0x7BCD                          # a finite 16-bit pattern in both dtypes
U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
WORST = {}


def _note(kind, dt, err, bound):
    k = (kind, dt)
    WORST[k] = max(WORST.get(k, 0.0), float(err / bound))
    print(f"{kind} {dt}: worst |error| {float(err):.3e}, bound {float(bound):.3e} (worst ratio so far {WORST[k]:.3f})")


def _attn_ref(q, k, v, heads, visible, scale=0.125):
    """q (B,Tq,C), k / v (B,Tk,C) float64; visible (Tq,Tk) bool -> (B,Tq,C)"""
    B, Tq, C = q.shape
    out = np.zeros((B, Tq, C))
    for h in range(heads):
        sl = slice(64 * h, 64 * h + 64)
        s = np.einsum("bid,bjd->bij", q[..., sl], k[..., sl]) * scale
        s = np.where(visible[None], s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        out[..., sl] = np.einsum("bij,bjd->bid", p / p.sum(-1, keepdims=True), v[..., sl])
    return out


# ------------------------------------------------------------------------------------------------------------------------------- prefix attention
PREFIX_CASES = sorted({(T, min(p, T)) for T in (1, 17, 64, 65, 130, 200) for p in (0, 1, 63, 64, 65, T)})


@pytest.fixture(scope="module")
def qkv_inputs():
    """one (B = 2, 200, 3C) fused buffer per dtype; a case of T tokens uses its first T rows per sample"""
    rng = np.random.default_rng(16)
    x = rng.standard_normal((2, 200, 3 * 128)).astype(np.float32)
    return {dt: to16(x, dt) for dt in ("f16", "bf16")}


def _run_attn(be, fn, bits, T, heads, dt, prefix=None, extra_rows=5, ldo_extra=64):
    B, C = bits.shape[0], heads * 64
    buf = be.dev(np.ascontiguousarray(bits[:, :T]))
    ldo = C + ldo_extra
    out = be.dev(np.full((B * T + extra_rows, ldo), SENT, np.uint16))
    p = be.ptr(buf)
    args = (p, 3 * C, p + 2 * C, 3 * C, p + 4 * C, 3 * C, be.ptr(out), ldo, B, T) + ((prefix,) if prefix is not None else (T,)) + (heads, 64, 0.125, DT[dt], be.stream)
    ok(fn(*args))
    be.sync()
    raw = be.host(out)
    assert (raw[:B * T, C:] == SENT).all(), "columns beyond heads * 64 were written"
    assert (raw[B * T:] == SENT).all(), "rows beyond B * T were written"
    return raw[:B * T, :C].reshape(B, T, C)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("T,prefix", PREFIX_CASES)
def test_prefix_attention(be, qkv_inputs, T, prefix, dt):
    """B = 2, heads = 2, q / k / v views of one (B T, 3C) buffer; key j reaches query i iff j < max(i + 1, prefix)"""
    heads, C = 2, 128
    bits, vals = qkv_inputs[dt]
    got_bits = _run_attn(be, be.lib.eegclip_self_attn_prefix_fwd, bits, T, heads, dt, prefix)
    x = vals[:, :T].astype(np.float64)
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    ref = _attn_ref(x[..., :C], x[..., C:2 * C], x[..., 2 * C:], heads, j < np.maximum(i + 1, prefix))
    got = from16(got_bits, dt).astype(np.float64)
    bound = 2 * U[dt] * np.abs(x[..., 2 * C:]).max() + 2e-4
    err = np.abs(got - ref).max()
    _note("prefix attention", dt, err, bound)
    assert np.isfinite(got).all() and err <= bound
    if prefix == 0:
        causal = _run_attn(be, be.lib.eegclip_self_attn_causal_fwd, bits, T, heads, dt)
        assert np.array_equal(causal, got_bits), "prefix = 0 is not the causal form bit for bit"
    if prefix == T:
        full = _run_attn(be, be.lib.eegclip_self_attn_fwd, bits, T, heads, dt)
        assert np.abs(from16(full, dt).astype(np.float64) - got).max() <= bound


def test_prefix_attention_rejections(be):
    C, T = 128, 16
    buf, out = be.zeros((1, T, 3 * C), np.uint16), be.zeros((1, T, C), np.uint16)
    p = be.ptr(buf)

    def fwd(prefix=3, T_=T, hd=64, dtype=1):
        return be.lib.eegclip_self_attn_prefix_fwd(p, 3 * C, p + 2 * C, 3 * C, p + 4 * C, 3 * C, be.ptr(out), C, 1, T_, prefix, 2, hd, 0.125, dtype, be.stream)

    assert fwd() == 0 and fwd(prefix=0) == 0 and fwd(prefix=T) == 0
    assert fwd(prefix=-1) == _abi_einval() and fwd(prefix=T + 1) == _abi_einval() and fwd(T_=0) < 0 and fwd(hd=80) < 0 and fwd(dtype=3) < 0


def _abi_einval():
    return -1                                                          # EEGCLIP_EINVAL (include/eegclip.h)


# ------------------------------------------------------------------------------------------------------------------------------- decode attention
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("B,heads", [(1, 1), (3, 12), (1, 12), (3, 1)])
def test_decode_attention(be, B, heads, Tk, dt):
    """one query row per sample from a (B, 3C) buffer against the first Tk rows of a (B, Tk + 7, 2C) cache whose unused rows are NaN"""
    rng = np.random.default_rng(1000 * B + 10 * heads + Tk)
    C, Tmax = heads * 64, Tk + 7
    q16, q = to16(rng.standard_normal((B, 3 * C)).astype(np.float32), dt)
    kv16, kv = to16(rng.standard_normal((B, Tmax, 2 * C)).astype(np.float32), dt)
    kv16 = kv16.copy()
    kv16[:, Tk:] = 0x7E00 if dt == "f16" else 0x7FC0                   # NaN in both halves of every unused row
    Q, KV = be.dev(q16), be.dev(kv16)
    out = be.dev(np.full((B + 2, C + 8), SENT, np.uint16))
    ok(be.lib.eegclip_decode_attn16(be.ptr(Q), 3 * C, be.ptr(KV), 2 * C, Tmax * 2 * C, be.ptr(out), C + 8, B, Tk, heads, 64, 0.125, DT[dt], be.stream))
    be.sync()
    raw = be.host(out)
    assert (raw[:B, C:] == SENT).all() and (raw[B:] == SENT).all(), "writes outside out[b, 0 .. C)"
    got = from16(raw[:B, :C], dt).astype(np.float64)
    k, v = kv[:, :Tk, :C].astype(np.float64), kv[:, :Tk, C:].astype(np.float64)
    ref = _attn_ref(q[:, None, :C].astype(np.float64), k, v, heads, np.ones((1, Tk), bool))[:, 0]
    bound = 2 * U[dt] * np.abs(v).max() + 2e-4
    err = np.abs(got - ref).max()
    _note("decode attention", dt, err, bound)
    assert np.isfinite(got).all(), "NaN from the unused cache rows reached the output"
    assert err <= bound


def test_decode_attention_rejections(be):
    C = 128
    q, kv, out = be.zeros((2, 3 * C), np.uint16), be.zeros((2, 9, 2 * C), np.uint16), be.zeros((2, C), np.uint16)

    def f(ldq=3 * C, ld_row=2 * C, ss=9 * 2 * C, Tk=9, hd=64, qoff=0, scale=0.125):
        return be.lib.eegclip_decode_attn16(be.ptr(q) + qoff, ldq, be.ptr(kv), ld_row, ss, be.ptr(out), C, 2, Tk, 2, hd, scale, 1, be.stream)

    assert f() == 0
    assert f(Tk=0) < 0 and f(hd=32) < 0 and f(ld_row=C) < 0 and f(ss=8 * 2 * C) < 0 and f(ldq=64) < 0 and f(scale=0.0) < 0
    assert f(qoff=2) < 0 and f(ldq=3 * C + 4) < 0


# ------------------------------------------------------------------------------------------------------------------------------- skinny GEMM
@pytest.fixture(scope="module")
def gemm_inputs():
    """A (16, 3072), W (2304, 3072), bias, R (16, 2304) per dtype; a case uses the leading M x K / N x K / M x N blocks"""
    rng = np.random.default_rng(7)
    a = rng.standard_normal((16, 3072)).astype(np.float32)
    w = rng.standard_normal((2304, 3072)).astype(np.float32)
    b = rng.standard_normal(2304).astype(np.float32)
    r = rng.standard_normal((16, 2304)).astype(np.float32)
    return {dt: tuple(to16(x, dt) for x in (a, w, b, r)) for dt in ("f16", "bf16")}


def _skinny(be, A, W, bias, R, M, N, K, c_f32, dt, ldc):
    out = be.dev(np.full((M, ldc), SENT, np.uint16)) if not c_f32 else be.dev(np.full((M, ldc), -7.0, np.float32))
    rc = be.lib.eegclip_gemm16_skinny(be.ptr(A), K, be.ptr(W), K, be.ptr(out), ldc, be.ptr(bias), be.ptr(R), N if R is not None else 0, M, N, K, int(c_f32), DT[dt],
                                      be.stream)
    be.sync()
    return rc, be.host(out)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("K", [64, 768, 3072])
@pytest.mark.parametrize("N", [1, 130, 515, 2304])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_skinny_gemm(be, gemm_inputs, M, N, K, dt):
    """none / bias / bias + R, 16-bit and fp32 output, ldc = N and ldc > N with sentinels between the rows; run to run bit-identical.  (W is scaled by
    1 / sqrt(K): results of order 1.)"""
    (a16, a), (w16, w), (b16, b), (r16, r) = gemm_inputs[dt]
    _check_skinny(be, a16, a, w, b16, b, r16, r, M, N, K, dt)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K,waves", [(5, 130, 256, 4), (5, 130, 512, 8), (2, 8200, 320, 8), (2, 16400, 320, 4), (1, 16400, 1088, 4)])
def test_skinny_gemm_every_wave_split(be, M, N, K, waves, dt):
    """the launch picks 4, 8 or 16 K-splitting waves from N / 16 and K / 64 (16: the cases above at K >= 768).  Here: 4 waves with one chunk each; 8 waves
    by K (8 chunks) and by N (513 workgroups; 5 chunks: three waves idle); 4 waves at >= 1024 workgroups, the LM head's form, with 5 chunks (wave 0 takes
    two) and with 17 (a second pass of the 4-chunk pipeline with three of its chunks past K)"""
    rng = np.random.default_rng(N + K)
    (a16, a), (b16, b), (r16, r) = (to16(rng.standard_normal(sh).astype(np.float32), dt) for sh in ((M, K), (N,), (M, N)))
    _check_skinny(be, a16, a, rng.standard_normal((N, K)).astype(np.float32), b16, b, r16, r, M, N, K, dt)


def _check_skinny(be, a16, a, w, b16, b, r16, r, M, N, K, dt):
    scale = np.float32(1.0 / np.sqrt(K))
    w16k, wk = to16(w[:N, :K] * scale, dt)
    A, W = be.dev(np.ascontiguousarray(a16[:M, :K])), be.dev(w16k)
    Bd, Rd = be.dev(np.ascontiguousarray(b16[:N])), be.dev(np.ascontiguousarray(r16[:M, :N]))
    a64, w64 = a[:M, :K].astype(np.float64), wk.astype(np.float64)
    prod, mag = a64 @ w64.T, np.abs(a64) @ np.abs(w64).T
    worst = {0: 0.0, 1: 0.0}
    # (epilogue, c_f32, ldc): each epilogue, both output types, ldc = N and ldc > N
    for mode, c_f32, ldc in ((0, 0, N), (1, 1, N + 9), (2, 0, N + 9), (2, 1, N)):
        bias, R = (None, Bd, Bd)[mode], (None, None, Rd)[mode]
        ref = prod + (b[:N] if mode else 0) + (r[:M, :N] if mode == 2 else 0)
        m = mag + (np.abs(b[:N]) if mode else 0) + (np.abs(r[:M, :N]) if mode == 2 else 0)
        f32_bound = (K + 2) * 2.0 ** -24 * m
        rc, raw = _skinny(be, A, W, bias, R, M, N, K, c_f32, dt, ldc)
        assert rc == 0
        assert (raw[:, N:] == (-7.0 if c_f32 else SENT)).all(), "columns >= N of a wider row were written"
        got = raw[:, :N].astype(np.float64) if c_f32 else from16(raw[:, :N], dt).astype(np.float64)
        bound = f32_bound if c_f32 else f32_bound + U[dt] * np.abs(ref) + 2.0 ** -24
        assert np.isfinite(got).all()
        ratio = (np.abs(got - ref) / np.maximum(bound, 1e-30)).max()
        worst[c_f32] = max(worst[c_f32], ratio)
        assert ratio <= 1.0, (mode, c_f32, ldc, ratio)
    rc, again = _skinny(be, A, W, Bd, Rd, M, N, K, 1, dt, N)
    assert rc == 0 and np.array_equal(again, raw), "two runs differ"
    print(f"skinny gemm M={M} N={N} K={K} {dt}: worst |error| / bound: 16-bit output {worst[0]:.3f}, fp32 output {worst[1]:.3f}")


def test_skinny_gemm_rejections(be):
    z = be.zeros((32, 128), np.uint16)
    c = be.zeros((32, 128), np.float32)

    def f(M=4, N=100, K=128, lda=128, ldw=128, ldc=128, c_f32=0, dtype=0, aoff=0):
        return be.lib.eegclip_gemm16_skinny(be.ptr(z) + aoff, lda, be.ptr(z), ldw, be.ptr(c), ldc, None, None, 0, M, N, K, c_f32, dtype, be.stream)

    assert f() == 0 and f(M=16) == 0 and f(c_f32=1) == 0
    assert f(M=17) == _abi_einval() and f(K=96, lda=96, ldw=96) == _abi_einval()
    assert f(M=0) < 0 and f(N=0) < 0 and f(ldc=64) < 0 and f(lda=64) < 0 and f(dtype=4) < 0 and f(c_f32=2) < 0
    assert f(aoff=2) < 0 and f(lda=132) < 0
