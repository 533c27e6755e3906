"""csrc/cross_attn.hip: SDXL cross-attention with the IP-Adapter branch (head_dim 64, S and S_ip <= 128 keys, 16-bit I/O) against the fp64 oracle on the
16-bit-rounded inputs, on the lane emulator and on the GPU.

Every run keeps 16 rows of NaN bit patterns behind the last row of q, k, v, k_ip and v_ip (same allocation) and 9 sentinel rows behind `out`: a read past an
operand shows as a non-finite or wrong output, a write past `out` as a changed sentinel.  Every test has >= 2 heads with different data.

Which kernel a (S, S_ip) pair runs: nt = ceil(S / 16) key tiles, nt_ip = ceil(S_ip / 16); nt == 5 with nt_ip <= 1 is the register kernel (its two-tile
lock step), everything else the generic one.  GRID reaches nt = 1 .. 8 (odd: the half-empty last k-step of P V), nt_ip = 0 .. 8, both V^T strides (68 halfs
up to 4 tiles, 132 above), S a multiple of 16 (no padding key) and 128 / 128, the largest LDS footprint the ABI admits (74,752 bytes).

Tolerances: tests/attn_models.py's cross_attn_model is the kernel's stated arithmetic (fp32 scores, normalised probabilities rounded to the I/O type, fp32
accumulation, one output rounding) on the CPU; `python tests/attn_models.py` measures it against fp64 on the exact inputs of every test here that compares
with the oracle.  MODEL below holds its worst max and worst mean error per group of cases; a test's atol and mean bound are 3x those (the margin
test_kernels_vae_attn.py gives for summation order: the kernel's sums are MFMA trees, the model's are fp64 sums rounded once), and never more than the
6e-3 / 2.5e-2 and a sixth of it that tests/test_kernels_ops.py's test has.  Two groups, told apart by the shape alone, because the error is the rounding of
an output whose size depends on how many keys a branch averages over:
  many_keys  every branch present has >= 48 keys, |out| < 1.6: atol 1.83e-3 (f16) / 1.44e-2 (bf16), mean 1.5e-4 / 1.2e-3.  The mean bound is what catches a
             mis-masked key on random inputs: three unmasked padding keys at S = 77 give a mean error of 3.3e-3 in both dtypes.
  few_keys   a branch with fewer keys (4 image tokens times ip_scale = 0.75 add a term of standard deviation 0.4; at S = 1 the output is v itself), |out|
             reaches 3.2 and its bf16 rounding alone 7.8e-3: atol 5.1e-3 / 2.5e-2 (3x the model would be 3.96e-2: the old bound stays), mean 3.9e-4 / 3.4e-3.
The stress cases have their own model figures: `large_negative` 2.85e-3 / 2.25e-2 and 3.2e-4 / 2.5e-3; `huge_scores` makes the softmax one-hot in both branches,
out = v[j] + 0.75 v_ip[j'] reaches 5.2, half a bf16 ulp of [4, 8) is 1.6e-2 whatever the kernel does, 3x the model would be 4.1e-2 and the old 2.5e-2 stays
(f16: 5.9e-3; means 5.1e-4 / 4.1e-3)."""
import numpy as np
import pytest
import torch

import attn_models as am
from backends import be, ok  # noqa: F401
from oracle import sdxl_attn

SENTINEL = 0x7BCD                      # a finite 16-bit pattern in both dtypes; never produced by the kernel for these inputs
NAN16 = 0x7FFF                         # a NaN in fp16 and in bf16
GUARD_ROWS, SENTINEL_ROWS = 16, 9
D = 64
DTYPES = pytest.mark.parametrize("f16", [True, False], ids=["f16", "bf16"])

# (S, S_ip): generic kernel nt = 1 .. 4 | register kernel, NT_IP = 0 and 1, with and without padding keys | generic kernel nt = 6 .. 8
GRID = [(1, 0), (15, 1), (16, 16), (17, 17), (33, 4), (48, 0), (64, 0),
        (77, 0), (77, 4), (77, 16), (65, 1), (80, 0),
        (81, 4), (96, 33), (113, 15), (128, 128)]


def _hw(S, S_ip):
    """a small HW in 40 .. 70 that is no multiple of 16 and differs between grid points"""
    hw = 40 + (7 * S + 3 * S_ip) % 31
    return hw + 1 if hw % 16 == 0 else hw


# (B, HW, heads, S, S_ip); HW = 530: a second workgroup in x (CA_QB = 512 queries each) with a partial tile; 580: the second workgroup's waves 1 .. 3 have a
# live tile (528 .. 575) whose lock-step partner (q0 + 64) lies wholly beyond HW
SHAPES = [(2, _hw(S, S_ip), 2, S, S_ip) for S, S_ip in GRID]
BIG_HW = [(1, 530, 2, 77, 4), (1, 580, 2, 77, 4)]


def _round16(a, f16):
    """float32 array -> (16-bit bit pattern as int16, the rounded values as float64)"""
    t16 = torch.tensor(np.asarray(a, np.float32)).to(torch.float16 if f16 else torch.bfloat16)
    return t16.view(torch.int16).numpy().copy(), t16.double().numpy()


def _from16(bits, f16):
    return torch.tensor(np.ascontiguousarray(bits)).view(torch.float16 if f16 else torch.bfloat16).double().numpy()


OLD = {True: (6e-3, 6e-3 / 6), False: (2.5e-2, 2.5e-2 / 6)}              # tests/test_kernels_ops.py's (atol, bound of the mean)
MODEL = {                                                                # worst (max, mean) error of cross_attn_model against fp64: f16, bf16
    "many_keys": ((6.1e-4, 5.0e-5), (4.8e-3, 4.0e-4)),
    "few_keys": ((1.7e-3, 1.3e-4), (1.32e-2, 1.14e-3)),
    "large_negative": ((9.5e-4, 1.07e-4), (7.5e-3, 8.2e-4)),
    "huge_scores": ((1.95e-3, 1.7e-4), (1.37e-2, 1.37e-3)),
}


def _bounds(group, f16):
    """(atol, bound of the mean) = 3x the model's worst, at most the old bound"""
    return tuple(min(3 * m, old) for m, old in zip(MODEL[group][0 if f16 else 1], OLD[f16]))


def _guarded(be, a16):
    """(B, T, C) bit patterns -> a device buffer of B * T + GUARD_ROWS rows, the guard rows NaN"""
    C = a16.shape[-1]
    buf = np.full((a16.shape[0] * a16.shape[1] + GUARD_ROWS, C), NAN16, np.int16)
    buf[:-GUARD_ROWS] = a16.reshape(-1, C)
    return be.dev(buf)


def _run(be, q, k, v, heads, f16, k_ip=None, v_ip=None, ip_scale=1.0, S_ip=None):
    """q (B,HW,C), k / v (B,S,C), k_ip / v_ip (B,S_ip,C) float32 -> (output values (B,HW,C), the rounded inputs (q, k, v, k_ip, v_ip), the raw out rows).
    S_ip = 0 with k_ip given: the image tokens are passed but not to be used."""
    B, HW, C = q.shape
    S = k.shape[1]
    ins = [q, k, v] + ([k_ip, v_ip] if k_ip is not None else [])
    r16 = [_round16(a, f16) for a in ins]
    bufs = [_guarded(be, bits) for bits, _ in r16]
    ptrs = [be.ptr(t) for t in bufs] + [None] * (5 - len(bufs))
    OUT = be.dev(np.full((B * HW + SENTINEL_ROWS, C), SENTINEL, np.int16))
    n_ip = (k_ip.shape[1] if k_ip is not None else 0) if S_ip is None else S_ip
    ok(be.lib.eegclip_cross_attn_fwd(*ptrs, be.ptr(OUT), B, HW, heads, D, S, n_ip, float(ip_scale), int(f16), be.stream))
    be.sync()
    del bufs
    raw = be.host(OUT)
    assert (raw[B * HW:] == SENTINEL).all(), "rows beyond B * HW were written"
    vals = [f for _, f in r16] + [None] * (5 - len(r16))
    return _from16(raw[:B * HW].reshape(B, HW, C), f16), vals, raw


def _check(got, ref, f16, group):
    atol, mean = _bounds(group, f16)
    err = np.abs(got - ref)
    print(f"max error {err.max():.3e} (atol {atol:.2e}), mean error {err.mean():.3e} (bound {mean:.2e}), max |ref| {np.abs(ref).max():.2f}")
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)
    assert err.mean() < mean


def _parity_inputs(B, HW, heads, S, S_ip, f16):
    rng = np.random.default_rng(100000 * B + 100 * HW + 7 * S + S_ip + 50000 * int(f16))
    C = heads * D
    q, k, v = (rng.standard_normal((B, T, C)).astype(np.float32) for T in (HW, S, S))
    k_ip, v_ip = (rng.standard_normal((B, S_ip, C)).astype(np.float32) for _ in range(2)) if S_ip else (None, None)
    return q, k, v, k_ip, v_ip


def _stress_inputs(case, f16):
    """test_kernels_self_attn.py's cases at S = 77, S_ip = 4: text scores near -60 (+- 1, the spread of the N(0, 1) parity inputs the tolerance was derived
    on) and image scores near -40, and |scores| ~ 1e9 in both branches"""
    rng = np.random.default_rng({"large_negative": 3, "huge_scores": 4}[case] + 10 * int(f16))
    B, HW, heads, S, S_ip = 2, 150, 2, 77, 4
    C = heads * D
    q, k, v = (rng.standard_normal((B, T, C)).astype(np.float32) for T in (HW, S, S))
    k_ip, v_ip = (rng.standard_normal((B, S_ip, C)).astype(np.float32) for _ in range(2))
    if case == "large_negative":
        q, k, k_ip = 0.3 * q, 0.3 * k, 0.3 * k_ip
        for h in range(heads):
            q[..., D * h] = 16.0                                                      # score ~ q[0] k[0] / 8 = 2 k[0]
            k[..., D * h] = -30.0 + 0.5 * rng.standard_normal((B, S)).astype(np.float32)
            k_ip[..., D * h] = -20.0 + 0.5 * rng.standard_normal((B, S_ip)).astype(np.float32)
    else:
        q, k, k_ip = (2e4 * a.clip(-2, 2) for a in (q, k, k_ip))
    return q, k, v, k_ip, v_ip, heads


def _model_case(inputs, heads, f16, ip_scale):
    def make():
        vals = [None if a is None else am.round16(a, f16) for a in inputs()[:5]]
        return am.cross_attn_model(*vals[:3], heads, vals[3], vals[4], ip_scale, f16), sdxl_attn.cross_attention(*vals[:3], heads, vals[3], vals[4], ip_scale)
    return make


MEMORY = [(2, 70, 2, 77, 4), (2, 70, 2, 33, 17)]                                 # test_memory_discipline's shapes


def _many_keys(S, S_ip):
    """does every branch average over >= 48 keys?  (see the docstring: the two tolerance classes)"""
    return S >= 48 and (S_ip == 0 or S_ip >= 48)


# what `python tests/attn_models.py` measures the model on: the exact inputs of every test here that goes through _check
MODEL_CASES = {
    **{name: [(f"{s}", f16, _model_case(lambda s=s, f16=f16: _parity_inputs(*s, f16), s[2], f16, 0.75))
              for s in SHAPES + BIG_HW + MEMORY if _many_keys(*s[3:]) == many for f16 in (True, False)]
       for name, many in (("many_keys", True), ("few_keys", False))},
    **{case: [(case, f16, _model_case(lambda case=case, f16=f16: _stress_inputs(case, f16), 2, f16, 0.75)) for f16 in (True, False)]
       for case in ("large_negative", "huge_scores")},
}


@DTYPES
@pytest.mark.parametrize("B,HW,heads,S,S_ip", SHAPES + BIG_HW, ids=lambda x: str(x))
def test_matches_oracle(be, B, HW, heads, S, S_ip, f16):
    q, k, v, k_ip, v_ip = _parity_inputs(B, HW, heads, S, S_ip, f16)
    got, (qf, kf, vf, kif, vif), _ = _run(be, q, k, v, heads, f16, k_ip, v_ip, ip_scale=0.75)
    _check(got, sdxl_attn.cross_attention(qf, kf, vf, heads, kif, vif, 0.75), f16, "many_keys" if _many_keys(S, S_ip) else "few_keys")


@DTYPES
@pytest.mark.parametrize("S,S_ip", GRID)
def test_every_key_counted_exactly_once(be, S, S_ip, f16):
    """q = 0 makes both attentions uniform; v[j] = S * onehot((j + h) mod 64) and v_ip[j] = S_ip * onehot((j + h + 32) mod 64) turn the output into the integer
    count of text keys per column plus ip_scale = 0.5 times the count of image keys: a dropped, duplicated or mis-masked key moves an entry by >= 0.5, an
    unmasked padding key (a zero row of V^T with probability 1 / 80 instead of 0) scales a whole row by 77 / 80.  S, S_ip <= 128 are exact in bf16; 1 / S
    rounded to bf16 costs at most 0.4 % of a count <= 2."""
    B, heads, HW = 2, 3, _hw(S, S_ip)
    rng = np.random.default_rng(1000 * S + S_ip + int(f16))
    C = heads * D
    q = np.zeros((B, HW, C), np.float32)
    k = rng.standard_normal((B, S, C)).astype(np.float32)
    v, count = am.count_values(B, S, heads, D)
    k_ip = v_ip = None
    if S_ip:
        k_ip = rng.standard_normal((B, S_ip, C)).astype(np.float32)
        v_ip, count_ip = am.count_values(B, S_ip, heads, D, shift=32)
        count = count + 0.5 * count_ip
    got, _, _ = _run(be, q, k, v, heads, f16, k_ip, v_ip, ip_scale=0.5)
    print(f"max error {np.abs(got - count).max():.3e}")
    np.testing.assert_allclose(got, np.broadcast_to(count, got.shape), rtol=0, atol=0.05)


def _onehot_case(B, HW, heads, S, S_ip):
    """k[j] = +-16 e_((j + h) mod n), q[i] = k[target(i)], target(i) = (5 i + h) mod S: the target scores 256 / 8 = 32, every other key 0 or -32, so the
    attention is one-hot up to e^-32 tails and the output is v[target], small integers that differ by key, column, head and sample.  With image tokens
    the text codes live in columns [0, ceil(S / 2)) and the image codes in the columns behind them, q = k[target] + k_ip[target_ip] selects one key in each
    branch without cross-talk, v_ip holds even integers and ip_scale = 0.5: out = v[target] + 0.5 v_ip[target_ip], exact in bf16.  There v is 0 .. 100 and
    v_ip / 2 is 0 .. 25, both NON-NEGATIVE: the two branches share fp32 accumulators and a matrix-core accumulation is not correctly rounded.  Measured on
    the MI355X with v and v_ip / 2 of both signs (-50 .. 50), bf16: in 37 of 67,840 entries, all of them with v[t] a power of two (1, 2, 8, 32) and
    v_ip[t'] / 2 = -v[t], the text branch's sum v[t] - (e^-32 tails) left the MFMA as the fp32 number just BELOW v[t], and the output was -2^-24 .. -2^-19
    instead of 0; every other entry was within 3e-12, and f16 (whose tails flush to 0) exact.  Without cancellation that last fp32 bit vanishes in the 16-bit
    output rounding, as it does in real use; an absolute 1e-6 on a DIFFERENCE of fp32 sums of size 32 is below what fp32 accumulation resolves (its ulp there
    is 3.8e-6) and is not what this test is about."""
    if not S_ip:
        k = am.onehot_keys(B, S, heads, D)
        v = am.int_values(B, S, heads, D)
        tgt = am.targets(HW, S, heads)
        return am.gather_rows(k, tgt, heads), k, v, None, None, am.gather_rows(v, tgt, heads).astype(np.float64)
    nt_cols, ni_cols = (S + 1) // 2, (S_ip + 1) // 2
    k = am.onehot_keys(B, S, heads, D, 0, nt_cols)
    k_ip = am.onehot_keys(B, S_ip, heads, D, nt_cols, ni_cols)
    v, v_ip = am.int_values(B, S, heads, D, lo=0), 2 * (am.int_values(B, S_ip, heads, D, lo=0) % 26)
    tgt, tgt_ip = am.targets(HW, S, heads), am.targets(HW, S_ip, heads, mul=3)
    q = am.gather_rows(k, tgt, heads) + am.gather_rows(k_ip, tgt_ip, heads)
    want = am.gather_rows(v, tgt, heads).astype(np.float64) + 0.5 * am.gather_rows(v_ip, tgt_ip, heads)
    return q, k, v, k_ip, v_ip, want


@DTYPES
@pytest.mark.parametrize("B,HW,heads,S,S_ip", [(1, 530, 2, 77, 0), (2, 70, 2, 80, 0), (1, 140, 3, 128, 0), (2, 40, 2, 17, 0), (1, 100, 2, 48, 0), (2, 45, 2, 96, 0),
                                               (1, 530, 2, 77, 4), (2, 70, 2, 77, 16), (2, 40, 2, 17, 17), (1, 100, 3, 96, 32), (1, 50, 2, 65, 1)],
                         ids=lambda x: str(x))
def test_each_query_returns_its_own_value_row(be, B, HW, heads, S, S_ip, f16):
    """a k-slot permutation between P and V^T, a wrong key tile, query tile, head or workgroup offset returns ANOTHER row's integers (an error of order 10),
    not a small error"""
    q, k, v, k_ip, v_ip, want = _onehot_case(B, HW, heads, S, S_ip)
    assert np.abs(want).max() <= 127
    got, (qf, kf, vf, kif, vif), _ = _run(be, q, k, v, heads, f16, k_ip, v_ip, ip_scale=0.5)
    ref = sdxl_attn.cross_attention(qf, kf, vf, heads, kif, vif, 0.5)
    np.testing.assert_allclose(ref, want, rtol=0, atol=1e-9, err_msg="the construction itself is no longer one-hot")
    print(f"max error {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


@DTYPES
@pytest.mark.parametrize("case", ["large_negative", "huge_scores"])
def test_softmax_stress(be, case, f16):
    """the kernel is single-pass and folds the scale into one FMA, exp2(s * c - mx * c) with c = log2(e) / 8, instead of subtracting first.  At |scores| ~ 1e9
    the rounding of mx * c alone is up to +-8 -- but it is the SAME for every key of the row, a common factor 2^+-8 that the normalisation removes: the result
    must be finite and right (see the docstring for the bound of that case)."""
    q, k, v, k_ip, v_ip, heads = _stress_inputs(case, f16)
    got, (qf, kf, vf, kif, vif), _ = _run(be, q, k, v, heads, f16, k_ip, v_ip, ip_scale=0.75)
    _check(got, sdxl_attn.cross_attention(qf, kf, vf, heads, kif, vif, 0.75), f16, case)


def _dirty_the_scratchpad(be):
    """a flash-attention launch on large NaN-free values first: on the emulator the next launch's LDS then holds them (not relied upon: the kernel must pass
    with any LDS content, this only makes a read of uninitialised LDS show up as a wrong or non-finite output here)"""
    big = be.dev(np.full((1, 64, 192), 0x7BFF, np.int16))          # fp16 65504 / a huge bf16
    out = be.zeros((1, 64, 64), np.int16)
    ok(be.lib.eegclip_self_attn_fwd(be.ptr(big), 192, be.ptr(big) + 128, 192, be.ptr(big) + 256, 192, be.ptr(out), 64, 1, 64, 64, 1, 64, 1e-6, 1, be.stream))
    be.sync()


@DTYPES
@pytest.mark.parametrize("B,HW,heads,S,S_ip", MEMORY, ids=["register_kernel", "generic_kernel"])
def test_memory_discipline(be, B, HW, heads, S, S_ip, f16):
    """NaN rows behind every operand and sentinel rows behind `out` (as in every run here), after a launch that left large values in the scratchpad: the
    output is finite and right; a second identical call gives the same bits; ip_scale = 0 with image tokens present equals the call without them"""
    _dirty_the_scratchpad(be)
    q, k, v, k_ip, v_ip = _parity_inputs(B, HW, heads, S, S_ip, f16)
    got, (qf, kf, vf, kif, vif), raw = _run(be, q, k, v, heads, f16, k_ip, v_ip, ip_scale=0.75)
    _check(got, sdxl_attn.cross_attention(qf, kf, vf, heads, kif, vif, 0.75), f16, "few_keys")
    assert np.array_equal(raw, _run(be, q, k, v, heads, f16, k_ip, v_ip, ip_scale=0.75)[2])
    without = _run(be, q, k, v, heads, f16)[0]
    assert np.array_equal(_run(be, q, k, v, heads, f16, k_ip, v_ip, ip_scale=0.0)[0], without)
    assert np.array_equal(_run(be, q, k, v, heads, f16, k_ip, v_ip, S_ip=0)[0], without)


def test_rejections(be):
    B, HW, heads, S, S_ip = 1, 16, 2, 16, 16
    C = heads * D
    buf = be.zeros((max(HW, 129) + 1, C), np.int16)
    OUT = be.dev(np.full((B * HW + 1, C), SENTINEL, np.int16))
    p, po = be.ptr(buf), be.ptr(OUT)

    def fwd(q=p, k=p, v=p, k_ip=p, v_ip=p, out=po, B_=B, HW_=HW, h=heads, hd=D, S_=S, S_ip_=S_ip, dtype=1):
        rc = be.lib.eegclip_cross_attn_fwd(q, k, v, k_ip, v_ip, out, B_, HW_, h, hd, S_, S_ip_, 0.5, dtype, be.stream)
        if rc < 0:
            be.sync()
            assert (be.host(OUT) == SENTINEL).all(), "a rejected call wrote to out"
        return rc

    for kw in ({"hd": 32}, {"hd": 128}, {"S_": 0}, {"S_": 129}, {"S_ip_": 129}, {"S_ip_": -1}, {"k_ip": None}, {"v_ip": None}, {"dtype": 7},
               {"B_": 0}, {"HW_": 0}, {"h": 0}, {"q": None}, {"k": None}, {"v": None}, {"out": None}):
        assert fwd(**kw) < 0, kw
    for name in ("q", "k", "v", "k_ip", "v_ip"):
        assert fwd(**{name: p + 2}) < 0, name                            # not 16-byte aligned
    assert fwd(out=po + 2) < 0
    assert fwd(k_ip=None, v_ip=None, S_ip_=0) == 0 and fwd() == 0       # (the arguments the rejections vary are otherwise fine)
    be.sync()
