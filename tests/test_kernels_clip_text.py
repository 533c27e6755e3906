"""The kernels added for SDXL's CLIP text encoders, on the lane emulator and on the GPU: the causal form of csrc/self_attn.hip against an fp64 masked
softmax, csrc/clip_text.hip's row gather (exact) and 16-bit activation (1 ulp)."""
import numpy as np
import pytest

from backends import be, ok  # noqa: F401
from test_kernels_self_attn import SENTINEL, _from16, _round16, _tol


# ------------------------------------------------------------------------------------------------------------------------ causal attention
def _attn(be, q, k, v, heads, f16, scale=0.125, fused=False, ldo_extra=0, extra_rows=0, causal=True):
    """q / k / v (B, T, C) float32 -> (output values (B, T, C), the rounded q / k / v as float64, the raw output buffer).  fused: one (B, T, 3C) buffer,
    strides 3C, bases offset by 0 / C / 2C elements."""
    B, T, C = q.shape
    q16, qf = _round16(q, f16)
    k16, kf = _round16(k, f16)
    v16, vf = _round16(v, f16)
    if fused:
        buf = np.zeros((B, T, 3 * C), np.int16)
        buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:] = q16, k16, v16
        QKV = be.dev(buf)
        bufs = (QKV,)
        pq, pk, pv = be.ptr(QKV), be.ptr(QKV) + 2 * C, be.ptr(QKV) + 4 * C
        ld = 3 * C
    else:
        bufs = (be.dev(q16), be.dev(k16), be.dev(v16))
        pq, pk, pv = (be.ptr(x) for x in bufs)
        ld = C
    ldo = C + ldo_extra
    OUT = be.dev(np.full((B * (T + extra_rows), ldo), SENTINEL, np.int16))
    fn = be.lib.eegclip_self_attn_causal_fwd if causal else be.lib.eegclip_self_attn_fwd
    ok(fn(pq, ld, pk, ld, pv, ld, be.ptr(OUT), ldo, B, T, T, heads, 64, float(scale), int(f16), be.stream))
    be.sync()
    del bufs
    raw = be.host(OUT)
    return _from16(raw[:B * T].reshape(B, T, ldo)[..., :C], f16), (qf, kf, vf), raw


def _ref(qf, kf, vf, heads, scale=0.125, causal=True):
    """fp64 softmax(scale q k^T + mask) v per head of 64"""
    B, T, C = qf.shape
    out = np.zeros((B, T, C))
    mask = np.triu(np.full((T, T), -np.inf), 1) if causal else np.zeros((T, T))
    for h in range(heads):
        s = slice(64 * h, 64 * h + 64)
        sc = np.einsum("bid,bjd->bij", qf[..., s], kf[..., s]) * scale + mask
        p = np.exp(sc - sc.max(-1, keepdims=True))
        out[..., s] = np.einsum("bij,bjd->bid", p / p.sum(-1, keepdims=True), vf[..., s])
    return out


def _check(got, ref, f16):
    tol = _tol(f16)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, atol=tol)
    assert np.abs(got - ref).mean() < tol / 6


@pytest.mark.parametrize("fused", [False, True], ids=["contiguous", "fused_qkv"])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("B,T,heads", [(1, 64, 1), (2, 77, 3), (1, 200, 2), (1, 257, 1)])
def test_causal_attention_matches_fp64(be, B, T, heads, f16, fused):
    rng = np.random.default_rng(B * 1000 + T * 7 + heads + 2 * int(f16) + int(fused))
    q, k, v = (rng.standard_normal((B, T, heads * 64)).astype(np.float32) for _ in range(3))
    got, (qf, kf, vf), _ = _attn(be, q, k, v, heads, f16, fused=fused)
    ref = _ref(qf, kf, vf, heads)
    _check(got, ref, f16)
    if T > 64:      # the flag is not ignored: the non-causal entry on the same inputs gives something else
        plain, _, _ = _attn(be, q, k, v, heads, f16, fused=fused, causal=False)
        _check(plain, _ref(qf, kf, vf, heads, causal=False), f16)
        assert np.abs(plain - got).max() > 5 * _tol(f16)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ["late_max", "early_max", "large_negative", "huge_scores"])
def test_online_softmax_stress_under_the_mask(be, case, f16):
    """tests/test_kernels_self_attn.py's stress inputs with the causal mask: the +40 scores of keys 192..199 ("late_max") now reach queries >= 192 only"""
    rng = np.random.default_rng({"late_max": 1, "early_max": 2, "large_negative": 3, "huge_scores": 4}[case] + 10 * int(f16))
    B, T, heads = 1, 200, 2
    C = heads * 64
    q = 0.3 * rng.standard_normal((B, T, C)).astype(np.float32)
    k = 0.3 * rng.standard_normal((B, T, C)).astype(np.float32)
    v = rng.standard_normal((B, T, C)).astype(np.float32)
    for h in range(heads):
        q[..., 64 * h] = 16.0
        if case == "late_max":
            k[:, 192:, 64 * h] = 20.0
        elif case == "early_max":
            k[:, :8, 64 * h] = 20.0
            k[:, 8:, 64 * h] = -5.0
        elif case == "large_negative":
            k[..., 64 * h] = -30.0 + 2.0 * rng.standard_normal((B, T)).astype(np.float32)
    if case == "huge_scores":
        q = 2e4 * rng.standard_normal((B, T, C)).astype(np.float32).clip(-2, 2)
        k = 2e4 * rng.standard_normal((B, T, C)).astype(np.float32).clip(-2, 2)
    got, (qf, kf, vf), _ = _attn(be, q, k, v, heads, f16)
    _check(got, _ref(qf, kf, vf, heads), f16)
    if case == "late_max":
        k2 = k.copy()
        for h in range(heads):
            k2[:, 192:, 64 * h] = 0.3 * rng.standard_normal((B, 8)).astype(np.float32)
        got2, _, raw2 = _attn(be, q, k2, v, heads, f16)
        _, _, raw = _attn(be, q, k, v, heads, f16)
        assert (raw[:192] == raw2[:192]).all(), "keys >= 192 reached a query < 192"
        assert np.abs(got[:, 192:] - got2[:, 192:]).max() > 5 * _tol(f16)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_causality_is_exact(be, f16):
    """k and v rows >= 60 changed: output rows < 60 bit-identical, rows >= 60 different; query 0 sees key 0 alone and returns v[0] to 16-bit rounding"""
    rng = np.random.default_rng(5 + int(f16))
    B, T, heads = 2, 77, 2
    C = heads * 64
    q, k, v = (rng.standard_normal((B, T, C)).astype(np.float32) for _ in range(3))
    got, (_, _, vf), raw = _attn(be, q, k, v, heads, f16)
    k2, v2 = k.copy(), v.copy()
    k2[:, 60:] = rng.standard_normal((B, T - 60, C)).astype(np.float32)
    v2[:, 60:] = rng.standard_normal((B, T - 60, C)).astype(np.float32) + 3.0
    got2, _, raw2 = _attn(be, q, k2, v2, heads, f16)
    raw, raw2 = raw.reshape(B, T, C), raw2.reshape(B, T, C)
    assert (raw[:, :60] == raw2[:, :60]).all()
    assert (np.abs(got[:, 60:] - got2[:, 60:]).max(-1) > _tol(f16)).all()
    ulp = 2.0 ** -10 if f16 else 2.0 ** -7
    np.testing.assert_allclose(got[:, 0], vf[:, 0], rtol=ulp, atol=1e-7)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_causal_attention_128_query_workgroups(be, f16):
    """B * heads * ceil(T / 128) = 512: the 128-query form, whose second key tile is wholly masked for the workgroup's first 64 queries (their running
    maximum, sum and accumulators must come through it unchanged)"""
    rng = np.random.default_rng(21 + int(f16))
    B, T, heads = 16, 200, 16
    assert B * heads * ((T + 127) // 128) >= 512
    q, k, v = (rng.standard_normal((B, T, heads * 64)).astype(np.float32) for _ in range(3))
    got, (qf, kf, vf), _ = _attn(be, q, k, v, heads, f16, fused=True)
    _check(got, _ref(qf, kf, vf, heads), f16)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_causal_writes_stay_inside_the_output_rows_and_heads(be, f16):
    rng = np.random.default_rng(11)
    B, T, heads, extra_rows, ldo_extra = 2, 70, 2, 9, 64
    C = heads * 64
    q, k, v = (rng.standard_normal((B, T, C)).astype(np.float32) for _ in range(3))
    got, (qf, kf, vf), raw = _attn(be, q, k, v, heads, f16, ldo_extra=ldo_extra, extra_rows=extra_rows)
    _check(got, _ref(qf, kf, vf, heads), f16)
    assert (raw[:B * T, C:] == SENTINEL).all(), "columns beyond heads*64 were written"
    assert (raw[B * T:] == SENTINEL).all(), "rows beyond B*T were written"


def test_causal_rejections(be):
    C, B, T, heads = 128, 1, 16, 2
    buf = be.zeros((B, T, 3 * C), np.int16)
    out = be.zeros((B, T, C), np.int16)
    p, po = be.ptr(buf), be.ptr(out)

    def fwd(hd=64, ld=C, ldo=C, B_=B, Tq=T, Tk=T, h=heads, q=p, scale=0.125, dtype=1):
        return be.lib.eegclip_self_attn_causal_fwd(q, ld, p, ld, p, ld, po, ldo, B_, Tq, Tk, h, hd, scale, dtype, be.stream)

    assert fwd(Tq=8) < 0 and fwd(Tk=8) < 0                             # Tq != Tk
    for hd in (40, 128):
        assert fwd(hd=hd) < 0
    assert fwd(ld=C + 4) < 0                                           # stride not a multiple of 8
    assert fwd(ldo=C + 2) < 0
    assert fwd(q=p + 2) < 0                                            # base not 16-byte aligned
    for kw in ({"B_": 0}, {"Tq": 0, "Tk": 0}, {"h": 0}):
        assert fwd(**kw) < 0
    assert fwd(ld=64) < 0                                              # stride shorter than heads * 64
    assert fwd(dtype=7) < 0 and fwd(scale=0.0) < 0 and fwd(scale=-0.125) < 0
    assert fwd() == 0


# ------------------------------------------------------------------------------------------------------------------------------ row gather
GUARD = 8                                                                # sentinel rows on either side of the table


@pytest.mark.parametrize("idx64", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("C", [128, 768, 1280])
def test_gather_rows16(be, C, f16, with_add, idx64):
    rng = np.random.default_rng(C + 2 * int(f16) + int(with_add) + 4 * int(idx64))
    rows_t, rows, add_rows = 50, 2 * 77, 77
    guarded = np.full((rows_t + 2 * GUARD, C), SENTINEL, np.int16)
    t16, tf = _round16(rng.standard_normal((rows_t, C)).astype(np.float32), f16)
    guarded[GUARD:GUARD + rows_t] = t16
    a16, af = _round16(rng.standard_normal((add_rows, C)).astype(np.float32), f16)
    idx = rng.integers(0, rows_t, rows)
    idx[:6] = [3, 3, 3, 0, rows_t - 1, rows_t - 1]                      # repeated, first and last
    T, A = be.dev(guarded), be.dev(a16)
    I = be.dev(idx.astype(np.int64 if idx64 else np.int32))
    OUT = be.dev(np.full((rows + 4, C), SENTINEL, np.int16))
    ok(be.lib.eegclip_gather_rows16(be.ptr(T) + 2 * GUARD * C, rows_t, be.ptr(I), int(idx64), be.ptr(A) if with_add else None, add_rows, be.ptr(OUT), rows, C,
                                    int(f16), be.stream))
    be.sync()
    raw = be.host(OUT)
    assert (raw[rows:] == SENTINEL).all(), "rows beyond `rows` were written"
    if with_add:
        want = (tf[idx].astype(np.float32) + af[np.arange(rows) % add_rows].astype(np.float32))       # one fp32 addition, rounded once
        want16, _ = _round16(want, f16)
        assert (raw[:rows] == want16).all()
    else:
        assert (raw[:rows] == t16[idx]).all()


@pytest.mark.parametrize("idx64", [False, True], ids=["int32", "int64"])
def test_gather_rows16_out_of_range_index_is_never_read_through(be, idx64):
    """indices outside [0, table_rows) are clamped to the table's first / last row: the sentinel rows around the table never reach the output"""
    C, rows_t = 128, 10
    guarded = np.full((rows_t + 2 * GUARD, C), SENTINEL, np.int16)
    t16, _ = _round16(np.arange(rows_t * C, dtype=np.float32).reshape(rows_t, C) % 251, True)
    guarded[GUARD:GUARD + rows_t] = t16
    idx = np.array([-1, rows_t, rows_t + 3, -GUARD, 2 ** 31 - 1, 4], np.int64)
    T, I = be.dev(guarded), be.dev(idx.astype(np.int64 if idx64 else np.int32))
    OUT = be.zeros((len(idx), C), np.int16)
    ok(be.lib.eegclip_gather_rows16(be.ptr(T) + 2 * GUARD * C, rows_t, be.ptr(I), int(idx64), None, 0, be.ptr(OUT), len(idx), C, 1, be.stream))
    be.sync()
    raw = be.host(OUT)
    assert not (raw == SENTINEL).any()
    assert (raw == t16[np.clip(idx, 0, rows_t - 1)]).all()


def test_gather_rows16_rejections(be):
    C = 128
    T, I, OUT = be.zeros((4, C), np.int16), be.zeros((4,), np.int64), be.zeros((4, C), np.int16)
    g = be.lib.eegclip_gather_rows16

    def call(table=None, tr=4, idx=None, i64=1, add=None, ar=0, out=None, rows=4, C_=C, dtype=1):
        return g(table or be.ptr(T), tr, idx or be.ptr(I), i64, add, ar, out or be.ptr(OUT), rows, C_, dtype, be.stream)

    assert call() == 0
    assert call(C_=100) < 0 and call(C_=0) < 0 and call(tr=0) < 0 and call(rows=0) < 0 and call(dtype=5) < 0 and call(i64=2) < 0
    assert call(add=be.ptr(T), ar=0) < 0                                # an added table without rows
    assert call(table=be.ptr(T) + 2) < 0 and call(out=be.ptr(OUT) + 4) < 0 and call(idx=be.ptr(I) + 4) < 0


# ------------------------------------------------------------------------------------------------------------------------------ activation
def _grid(f16):
    big = 6e4 if f16 else 3e38
    tiny = 2.0 ** -24 if f16 else 2.0 ** -133                            # subnormal in the dtype
    pts = [0.0, -0.0, 1.0, -1.0, 30.0, -30.0, big, -big, tiny, -tiny, 3 * tiny, 2.0 ** -15, -2.0 ** -15, 0.5, -0.5, 2.5, -2.5, 5.0, -5.0, 8.0, -8.0]
    x = np.concatenate([np.array(pts), np.linspace(-12, 12, 1027)]).astype(np.float32)
    return np.concatenate([x, np.zeros(-len(x) % 8, np.float32)])


def _act_ref(x, kind):
    import math
    x = np.asarray(x, np.float64)
    if kind == 0:
        with np.errstate(over="ignore"):
            return x / (1.0 + np.exp(-1.702 * x))
    return 0.5 * x * np.array([math.erfc(-t / math.sqrt(2.0)) for t in x])       # (erfc: no cancellation in the negative tail)


def _ulp(v, f16):
    """spacing of the 16-bit format at |v| (the subnormal spacing below the smallest normal)"""
    mant, emin = (10, -14) if f16 else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** emin)))
    return 2.0 ** (e - mant)


def _act(be, x16, kind, f16, inplace=False, ldx=None, ldy=None):
    M, D = x16.shape
    ldx, ldy = ldx or D, ldy or D
    xb = np.full((M, ldx), SENTINEL, np.int16)
    xb[:, :D] = x16
    X = be.dev(xb)
    Y = X if inplace else be.dev(np.full((M, ldy), SENTINEL, np.int16))
    ok(be.lib.eegclip_act16(be.ptr(X), ldx, be.ptr(Y), ldx if inplace else ldy, M, D, kind, int(f16), be.stream))
    be.sync()
    return be.host(Y)


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_act16_matches_fp64_to_one_ulp(be, f16):
    """quick_gelu (0) and erf gelu (1) on a grid with +-0, +-30, +-the format's largest magnitudes and subnormals: |error| <= 1 ulp of the output + 1e-6;
    the two kinds are further apart than that (0.8458 / 0.8413 at x = 1, -0.1542 / -0.1587 at x = -1)"""
    x16, xf = _round16(_grid(f16), f16)
    x16, xf = x16.reshape(-1, 8), xf.reshape(-1, 8)
    got = {}
    for kind in (0, 1):
        raw = _act(be, x16, kind, f16)
        got[kind] = _from16(raw, f16)
        ref = _act_ref(xf.ravel(), kind).reshape(xf.shape)
        assert np.isfinite(got[kind]).all()
        err = np.abs(got[kind] - ref)
        assert (err <= _ulp(ref, f16) + 1e-6).all(), (kind, float(err.max()), xf.ravel()[err.argmax()])
        assert (_act(be, x16, kind, f16, inplace=True) == raw).all()      # in place: the same bits
    one = np.argmin(np.abs(xf.ravel() - 1.0))
    mone = np.argmin(np.abs(xf.ravel() + 1.0))
    for i, (a, b) in ((one, (0.8458, 0.8413)), (mone, (-0.1542, -0.1587))):     # x sigmoid(1.702 x) and x Phi(x) at x = 1, -1 to four digits
        g0, g1 = got[0].ravel()[i], got[1].ravel()[i]
        assert abs(g0 - a) < 5e-5 + _ulp(a, f16) and abs(g1 - b) < 5e-5 + _ulp(b, f16)
        assert abs(g0 - g1) > _ulp(a, f16) + 1e-6
    diff = np.abs(got[0] - got[1])
    assert (diff > _ulp(got[0], f16) + 1e-6).sum() > len(diff.ravel()) // 4         # the kinds differ over the grid, not at two points only


@pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])
def test_act16_strides_and_bounds(be, f16):
    """row strides wider than D: columns >= D of the output keep their sentinel, columns >= D of the input are not read into it"""
    rng = np.random.default_rng(3)
    M, D = 5, 40
    x16, xf = _round16(rng.standard_normal((M, D)).astype(np.float32) * 3, f16)
    raw = _act(be, x16, 1, f16, ldx=56, ldy=48)
    assert (raw[:, D:] == SENTINEL).all()
    assert (raw[:, :D] == _act(be, x16, 1, f16)).all()


def test_act16_rejections(be):
    X = be.zeros((4, 64), np.int16)
    f = be.lib.eegclip_act16
    p = be.ptr(X)
    assert f(p, 64, p, 64, 4, 64, 0, 1, be.stream) == 0
    assert f(p, 64, p, 64, 4, 64, 2, 1, be.stream) < 0 and f(p, 64, p, 64, 4, 64, 0, 3, be.stream) < 0
    assert f(p, 64, p, 64, 4, 60, 0, 1, be.stream) < 0 and f(p, 32, p, 64, 4, 64, 0, 1, be.stream) < 0 and f(p, 68, p, 64, 4, 64, 0, 1, be.stream) < 0
    assert f(p + 2, 64, p, 64, 4, 64, 0, 1, be.stream) < 0 and f(p, 64, p, 64, 0, 64, 0, 1, be.stream) < 0
