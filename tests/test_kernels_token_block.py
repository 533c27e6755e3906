"""csrc/token_block.hip through the C ABI on both backends, tensor by tensor, against the fp64 reference of tests/token_block_ref.py:
eegclip_token_block_fwd (every output, every optional branch of the descriptor: stored n2, no xp, joint-subject embeddings with both bias strides, token
ids, arbitrary dropout sites, 64-bit seeds, drop_p 0 / 0.25 / 0.9) and eegclip_token_block_bwd parts 0, 1 and 2, in four input regimes (benign / offset /
sharp / sparse, token_block_ref.make_case).

Two comparisons per tensor, both elementwise against bounds derived in token_block_ref.py (no element is left out, no max-scaled tolerance for a stage):
  stage       the kernel's output against fp64 of the SAME operation on the kernel's own input to that stage (qkv from the kernel's h, f1 from the decoded n1
              planes, ...), bound c 2^-16 (|x| |W|^T + |b|) for a Linear, the fp32 round-off scales for LayerNorm / softmax / GELU
  end to end  against the whole fp64 chain, tolerance 4 x the drift of the fp32 split-bf16 model of the chain, measured on the CPU per regime and tensor and
              recorded in token_block_ref.E2E_DRIFT (independent of the kernel)
Every output buffer lies inside a larger allocation, NaN-filled between two canaries: every element must be written and finite, nothing outside may change,
a buffer the contract leaves alone must still be NaN, read-only inputs must be bit-identical afterwards.

TOKEN_BLOCK_REPORT=<file>: the worst observed error / bound per tensor is written there as JSON (what the pull request's summary quotes)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import token_block_ref as ref
from backends import BACKENDS, be  # noqa: F401
from eeg_image_decode_amd import _abi
from token_block_ref import D, FF, HE, L, NCH, T, bf16_round, decode_planes, split

EINVAL, EALIGN = -1, -2
SEEDS = (0x2A, 0x9E3779B97F4A7C15)                             # a small one, one with bits 32 - 63 set
SITES = ((0, 1, 2, 3, 4), (11, 3, 200, 7, 5))                  # the product's five ids, a permuted non-contiguous set
IDS = {1: [9], 2: [9, 0], 3: [9, 0, 9]}                        # a repeated row, the first and the last row of the 10-row table
SUBJ = {1: [2], 2: [2, 0], 3: [2, 0, 2]}
CANARY_F, CANARY_P, NAN_P = np.float32(-7777.25), 0xC3C3, 0x7FC0
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TOKEN_BLOCK_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({k: round(v, 4) for k, v in sorted(REPORT.items())}, f, indent=1)


# ---- guarded buffers ---------------------------------------------------------------------------------------------------------------------
class Out:
    """n elements (fp32, or bf16 bits for token planes) behind and in front of 64 floats' worth of canary; interior NaN unless `init` is given"""

    def __init__(self, be, n, planes=False, init=None):
        self.be, self.n, self.planes = be, int(n), planes
        self.pad = 128 if planes else 64                       # 256 bytes: the 16-byte alignment of the allocation carries over
        a = np.empty(self.n + 2 * self.pad, np.uint16 if planes else np.float32)
        a[:] = CANARY_P if planes else CANARY_F
        if init is not None:
            a[self.pad:self.pad + self.n] = np.asarray(init).reshape(-1)
        elif planes:
            a[self.pad:self.pad + self.n] = NAN_P
        else:
            a[self.pad:self.pad + self.n] = np.nan
        self.d = be.dev(a)
        self.ptr = be.ptr(self.d) + self.pad * a.itemsize
        assert self.ptr % 16 == 0

    def read(self, written=True):
        a = self.be.host(self.d)
        can = np.uint16(CANARY_P) if self.planes else CANARY_F
        assert (a[:self.pad] == can).all() and (a[self.pad + self.n:] == can).all(), "a canary next to the buffer was overwritten"
        v = a[self.pad:self.pad + self.n]
        if self.planes:
            nan = (v & 0x7F80) == 0x7F80
        else:
            nan = ~np.isfinite(v)
        if written:
            assert not nan.any(), f"{int(nan.sum())} elements not written or not finite"
        else:
            assert (v == NAN_P).all() if self.planes else np.isnan(v).all(), "a buffer the contract leaves alone was written"
        return v.copy()


class Ins:
    """read-only inputs: uploaded once, bit-identical afterwards"""

    def __init__(self, be):
        self.be, self.h, self.d = be, {}, {}

    def add(self, name, a):
        a = np.ascontiguousarray(a)
        self.h[name], self.d[name] = a, self.be.dev(a)
        return self.be.ptr(self.d[name])

    def check(self):
        for k, a in self.h.items():
            got = self.be.host(self.d[k])
            assert got.tobytes() == a.tobytes(), f"read-only input {k} changed"


def pack_weights(be, ins, P, joint):
    lib = be.lib
    packed = be.dev(np.zeros(int(lib.eegclip_token_block_packed_bytes()) // 2, np.uint16))
    # (joint model: the matrix in `packed` must not be used -- it is packed from NaNs)
    wv = np.full((D, T), np.nan, np.float32) if joint else P["wv"]
    w = [be.dev(np.ascontiguousarray(v)) for v in (wv, P["wqkv"], P["wo"], P["w1"], P["w2"])]
    assert lib.eegclip_token_block_pack(*[be.ptr(v) for v in w], be.ptr(packed), be.stream) == 0
    pe = None
    if joint:
        S = P["wv"].shape[0]
        pe = be.dev(np.zeros(int(lib.eegclip_token_block_packed_embed_bytes(S)) // 2, np.uint16))
        wj = be.dev(np.ascontiguousarray(P["wv"]))
        assert lib.eegclip_token_block_pack_embed(be.ptr(wj), D * T, S, be.ptr(pe), be.stream) == 0
    be.sync()
    ins.h["packed"], ins.d["packed"] = be.host(packed).copy(), packed
    if joint:
        ins.h["packed_embed"], ins.d["packed_embed"] = be.host(pe).copy(), pe
    return packed, pe


# ---- comparison --------------------------------------------------------------------------------------------------------------------------
class Checker:
    def __init__(self, tag):
        self.tag, self.fail = tag, []

    def close(self, name, got, want, bound, kind="stage"):
        got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.isfinite(want).all() and np.isfinite(bound).all(), name + ": the reference must be finite everywhere"
        err = np.abs(got - want)
        err = np.where(np.isfinite(err), err, np.inf)
        zero = bound == 0
        ratio = float(np.max(np.where(zero, np.where(err == 0, 0.0, np.inf), err / np.where(zero, 1.0, bound)))) if err.size else 0.0
        key = f"{kind}:{name}"
        REPORT[key] = max(REPORT.get(key, 0.0), ratio)
        print(f"{self.tag} {key:24s} error / bound = {ratio:.3f}   (max |err| {float(err.max()):.3e}, max |ref| {float(np.abs(want).max()):.3e})")
        if not ratio <= 1.0:
            self.fail.append(f"{key}: error / bound = {ratio:.3f} at {np.unravel_index(int(np.argmax(err / np.where(zero, 1e-300, bound))), err.shape)}")

    def equal(self, name, got, want):
        got = np.asarray(got)
        want = np.broadcast_to(np.asarray(want), got.shape)
        if not np.array_equal(got, want):
            self.fail.append(f"{name}: not bit-identical ({int((np.asarray(got) != np.asarray(want)).sum())} elements differ)")

    def done(self):
        assert not self.fail, self.tag + "\n" + "\n".join(self.fail)


def plane_properties(ck, name, hi, lo, width, ones, zero_row0=False, head_gaps=False):
    """hi == bf16(hi + lo); channels past the tensor's width exactly 0 in both planes; channel 255: 1 | 0 where the tensor carries the bias-gradient column"""
    # (hi is A nearest bf16 of hi + lo: where lo is exactly half a spacing the sum is a tie, and round-to-even of the sum may name the other neighbour)
    s = hi.astype(np.float64) + lo.astype(np.float64)
    r = bf16_round(s.astype(np.float32)).reshape(hi.shape)
    ck.equal(name + ": hi = bf16(hi + lo)", (r == hi) | (np.abs(s - hi) == np.abs(s - r)), True)
    pad = np.zeros(256, bool)
    if head_gaps:
        pad[[64 * h + d for h in range(4) for d in (62, 63)]] = True
    else:
        pad[width:] = True
    if ones:
        pad[255] = False
        r0 = 1 if zero_row0 else 0
        ck.equal(name + ": ones column", np.stack([hi[:, r0:, 255], lo[:, r0:, 255]]), np.stack([np.ones_like(hi[:, r0:, 255]), np.zeros_like(hi[:, r0:, 255])]))
    ck.equal(name + ": padding channels are zero", np.stack([hi[:, :, pad], lo[:, :, pad]]), 0.0)
    if zero_row0:
        ck.equal(name + ": token row 0 is zero", np.stack([hi[:, 0], lo[:, 0]]), 0.0)


def e2e_tolerance(regime, k, r, plane=False):
    """4 x the recorded drift of the fp32 split-bf16 model from the fp64 chain for this regime and tensor (token_block_ref.E2E_DRIFT, relative to max |ref|;
    + the resolution of a plane pair for tensors that leave as planes)"""
    return (4.0 * ref.E2E_DRIFT[regime][k] + (ref.PLANE if plane else 0.0)) * float(np.abs(r).max())


# ---- forward -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def forward_reference(regime, B, p, seed, sites, ids, joint_stride):
    P, x = ref.make_case(regime, B, n_subjects=3 if joint_stride else 0, bv_stride=joint_stride or D)
    masks = ref.make_masks(seed, sites, B, p)
    idv = IDS[B] if ids else None
    sj = SUBJ[B] if joint_stride else None
    R = ref.forward(P, x, idv, sj, masks, p)
    return P, x, masks, R


def run_forward(be, P, x, B, p, seed, sites, ids, joint_stride, store_n2, write_xp, eps=ref.EPS, scale=ref.SCALE):
    ins = Ins(be)
    packed, pembed = pack_weights(be, ins, P, bool(joint_stride))
    o = {k: Out(be, B * L * w) for k, w in (("h", D), ("qkv", 3 * HE), ("r1", D), ("f1", FF), ("r2", D), ("n2", D), ("n3", D))}
    o.update({k: Out(be, B * L) for k in ("mu1", "rs1", "mu2", "rs2", "mu3", "rs3")})
    o.update({k: Out(be, B * 32768, planes=True) for k in ("xp", "hp", "ctxp", "n1p", "g1p")})
    d = _abi.TokenBlockDesc(
        B=B, x=ins.add("x", x), packed=be.ptr(packed), bv=ins.add("bv", P["bv"]), pe=ins.add("pe", P["pe"]), tokens=ins.add("tokens", P["tokens"]),
        ids=ins.add("ids", np.asarray(IDS[B], np.int64)) if ids else None,
        **{k: ins.add(k, P[k]) for k in ("bqkv", "bo", "ln1_g", "ln1_b", "b1", "b2", "ln2_g", "ln2_b", "ln3_g", "ln3_b")},
        **{k: o[k].ptr for k in o if k not in ("n2", "xp")}, n2=o["n2"].ptr if store_n2 else None, xp=o["xp"].ptr if write_xp else None,
        drop_p=p, eps=eps, scale=scale, seed=seed, site_embed=sites[0], site_attn=sites[1], site_attn_out=sites[2], site_ffn_act=sites[3], site_ffn_out=sites[4],
        packed_embed=be.ptr(pembed) if joint_stride else None, embed_subject=ins.add("subj", np.asarray(SUBJ[B], np.int32)) if joint_stride else None,
        bv_stride=joint_stride or 0)
    assert be.lib.eegclip_token_block_fwd(ctypes.byref(d), be.stream) == 0
    be.sync()
    K = {k: v.read(written=not ((k == "n2" and not store_n2) or (k == "xp" and not write_xp))) for k, v in o.items()}
    ins.check()
    return K


def check_forward(tag, regime, K, P, x, masks, R, B, p, ids, joint_stride, store_n2, write_xp):
    ck = Checker(tag)
    f64 = lambda a: np.asarray(a, np.float64)
    W = {k: f64(v) for k, v in P.items()}
    ksc = ref.drop_scale(p) if p > 0 else 1.0
    mk = (lambda nm: masks[nm] * ksc) if masks is not None else (lambda nm: 1.0)
    Rn = {k: v.detach().numpy() for k, v in R.items()}
    if p >= 0.9:                                               # neither empty nor trivial
        for nm, m in masks.items():
            assert 0.05 <= m.mean() <= 0.15, (nm, m.mean())
    assert all(np.isfinite(v).all() for v in Rn.values())      # (sharp: the reference itself is finite everywhere)
    h = K["h"].reshape(B, L, D)
    qkv = K["qkv"].reshape(B, L, 3 * HE)
    # -- planes: layout properties, then values
    ctx, chi, clo = decode_planes(K["ctxp"], B, HE, heads=True)
    n1, nhi, nlo = decode_planes(K["n1p"], B)
    g1, ghi, glo = decode_planes(K["g1p"], B, FF)
    _, hhi, hlo = decode_planes(K["hp"], B)
    plane_properties(ck, "hp", hhi, hlo, D, ones=True)
    plane_properties(ck, "ctxp", chi, clo, HE, ones=True, head_gaps=True)
    plane_properties(ck, "n1p", nhi, nlo, D, ones=True)
    plane_properties(ck, "g1p", ghi, glo, FF, ones=False)
    eh, el = split(h.reshape(-1, D))                           # the h planes are the split of the fp32 h the same launch wrote, exactly
    ck.equal("hp = split(h)", np.stack([hhi[:, :, :D], hlo[:, :, :D]]), np.stack([eh.reshape(B, L, D), el.reshape(B, L, D)]))
    if write_xp:
        _, xhi, xlo = decode_planes(K["xp"], B)
        plane_properties(ck, "xp", xhi, xlo, D, ones=True, zero_row0=True)
        eh, el = split(x.reshape(-1, T))
        ck.equal("xp = split(x)", np.stack([xhi[:, 1:, :T], xlo[:, 1:, :T]]), np.stack([eh.reshape(B, NCH, T), el.reshape(B, NCH, T)]))
    # -- h: token row 0 exactly; the embedding rows against the Linear bound; the keep pattern
    idv = np.asarray(IDS[B] if ids else [0] * B)
    ksc32 = np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)
    tok = P["tokens"][idv] * ksc32
    ck.equal("h: token row", h[:, 0], np.where(masks["embed"][:, 0], tok, np.float32(0.0)) if masks is not None else tok)
    if p >= 0.9:
        ck.equal("h: zeros exactly where the mask drops", h != 0, masks["embed"])
    if joint_stride:
        sj = SUBJ[B]
        hb = np.stack([ref.lin_bound(f64(x[b]), W["wv"][sj[b]], np.abs(W["bv"][sj[b], :D]) + np.abs(W["pe"])) for b in range(B)])
    else:
        hb = ref.lin_bound(f64(x), W["wv"], np.abs(W["bv"]) + np.abs(W["pe"]))
    ck.close("h", h[:, 1:], Rn["h"][:, 1:], hb * (mk("embed")[:, 1:] if masks is not None else 1.0))
    # -- q | k | v from the kernel's h
    hk = f64(h)
    ck.close("qkv", qkv, hk @ W["wqkv"].T + W["bqkv"], ref.lin_bound(hk, W["wqkv"], W["bqkv"]))
    # -- attention from the kernel's q | k | v
    cr, Pd, s = ref.attention(ref.Arith(False), ref.t64(qkv), None if masks is None else torch.from_numpy(masks["attn"]), ksc, ref.SCALE)
    ck.close("ctx", ctx, cr.numpy(), ref.attention_bound(f64(qkv), Pd.numpy(), s.numpy(), ksc) + ref.PLANE * np.abs(cr.numpy()))
    # -- r1 from the kernel's h and ctx planes
    r1 = f64(K["r1"]).reshape(B, L, D)
    want = hk + mk("attn_out") * (ctx @ W["wo"].T + W["bo"])
    ck.close("r1", r1, want, mk("attn_out") * ref.lin_bound(ctx, W["wo"], W["bo"]) + 2 * ref.U24 * (np.abs(hk) + np.abs(want)))
    # -- LayerNorm 1 from the kernel's r1
    y, mu, rs, by, bm, br = ref.ln_bounds(r1, W["ln1_g"], W["ln1_b"])
    ck.close("n1", n1, y, by + ref.PLANE * np.abs(y))
    ck.close("mu1", K["mu1"].reshape(B, L), mu, bm)
    ck.close("rs1", K["rs1"].reshape(B, L), rs, br)
    # -- FFN from the decoded n1 planes / the kernel's f1 / the decoded g1 planes
    f1 = f64(K["f1"]).reshape(B, L, FF)
    ck.close("f1", f1, n1 @ W["w1"].T + W["b1"], ref.lin_bound(n1, W["w1"], W["b1"]))
    ge = ref.gelu(ref.t64(f1)).numpy()
    ck.close("g1", g1, ge * mk("ffn_act"), (ref.gelu_bound(f1, ge) + ref.PLANE * np.abs(ge)) * mk("ffn_act"))
    r2 = f64(K["r2"]).reshape(B, L, D)
    want = n1 + mk("ffn_out") * (g1 @ W["w2"].T + W["b2"])
    ck.close("r2", r2, want, mk("ffn_out") * ref.lin_bound(g1, W["w2"], W["b2"]) + ref.PLANE * np.abs(n1) + 2 * ref.U24 * (np.abs(n1) + np.abs(want)))
    # -- LayerNorm 2 from the kernel's r2, the final LayerNorm from the kernel's n2 (stored) or through the bound of the one re-evaluated here
    y2, mu, rs, by2, bm, br = ref.ln_bounds(r2, W["ln2_g"], W["ln2_b"])
    ck.close("mu2", K["mu2"].reshape(B, L), mu, bm)
    ck.close("rs2", K["rs2"].reshape(B, L), rs, br)
    if store_n2:
        n2 = f64(K["n2"]).reshape(B, L, D)
        ck.close("n2", n2, y2, by2)
        by2 = 0.0 * by2
    else:
        n2 = y2
    y3, mu, rs, by3, bm, br = ref.ln_bounds(n2, W["ln3_g"], W["ln3_b"])
    rs_ = rs[..., None]
    xh = (n2 - mu[..., None]) * rs_
    ck.close("n3", f64(K["n3"]).reshape(B, L, D), y3, by3 + ref.ln_perturb(by2, xh, W["ln3_g"], rs_))
    ck.close("mu3", K["mu3"].reshape(B, L), mu, bm + np.mean(by2, -1))
    ck.close("rs3", K["rs3"].reshape(B, L), rs, br + rs * rs * np.mean(np.abs(xh) * (by2 + np.mean(by2, -1, keepdims=True)), -1))
    # -- end to end
    got = {"h": h, "qkv": qkv, "ctx": ctx, "r1": r1, "n1": n1, "f1": f1, "g1": g1, "r2": r2, "n3": K["n3"].reshape(B, L, D)}
    got.update({k: K[k].reshape(B, L) for k in ("mu1", "rs1", "mu2", "rs2", "mu3", "rs3")})
    if store_n2:
        got["n2"] = K["n2"].reshape(B, L, D)
    for k, v in got.items():
        ck.close(k, v, Rn[k], e2e_tolerance(regime, k, Rn[k], plane=k in ("ctx", "n1", "g1")), kind="e2e")
    ck.done()


def forward_cases():
    """regime x B x drop_p in full; the other switches of the descriptor rotate through them so that every value meets every regime and every drop_p
    (a full cross product would be 2304 launches).  (regime, B, p, seed, sites, ids, joint bv_stride or 0, store n2, write xp)"""
    cases = []
    for r, regime in enumerate(("benign", "offset", "sharp", "sparse")):
        for j, (B, p) in enumerate((B, p) for B in (1, 3) for p in (0.0, 0.25, 0.9)):
            i = j + r
            cases.append(pytest.param(regime, B, p, SEEDS[i % 2], SITES[(i // 2 + j) % 2], bool((i + j // 3) % 2), (0, D, 252)[(i + r) % 3], bool((j + r // 2) % 2),
                                      bool((i // 3 + r) % 2), id=f"{regime}-B{B}-p{p}-{j}"))
    return cases


@pytest.mark.parametrize("regime,B,p,seed,sites,ids,joint_stride,store_n2,write_xp", forward_cases())
def test_forward_against_the_fp64_reference(be, regime, B, p, seed, sites, ids, joint_stride, store_n2, write_xp):
    if be.name == "emu" and B > 2:
        B = 2                                                  # the emulator runs a workgroup in ~10 s; the flat dropout index still starts past 0 for sample 1
    P, x, masks, R = forward_reference(regime, B, p, seed, sites, ids, joint_stride)
    if regime == "sharp":                                      # the regime is what it claims to be: +-60 in every head, a few logits past exp's fp32 overflow point
        s = R["logits"].detach().numpy()
        assert all(np.abs(s[:, hd]).max() >= 60.0 for hd in range(4)) and (s[:, 0] > 90.0).sum() >= 3
        assert (torch.softmax(R["logits"].detach(), -1).max(-1).values > 0.99).float().mean() > 0.5       # near-one-hot rows
    if regime == "offset" and p == 0.0:                        # rows whose mean dwarfs their spread, in r1 and in r2 (dropout zeroes a quarter of any offset)
        for k in ("r1", "r2"):
            v = R[k].detach().numpy()
            assert (np.abs(v.mean(-1)) >= 50.0 * v.std(-1)).sum() >= 8, k
    K = run_forward(be, P, x, B, p, seed, sites, ids, joint_stride, store_n2, write_xp)
    check_forward(f"[{be.name} {regime} B={B} p={p}]", regime, K, P, x, masks, R, B, p, ids, joint_stride, store_n2, write_xp)


def test_forward_is_independent_of_the_batch(be):
    """evaluation mode: a sample's outputs are bit-identical launched alone and as the last sample of a batch of 3"""
    P, x = ref.make_case("benign", 3)
    a = run_forward(be, P, x, 3, 0.0, 1, SITES[0], False, 0, True, True)
    b = run_forward(be, P, x[2:], 1, 0.0, 1, SITES[0], False, 0, True, True)
    for k, v in a.items():
        n = v.size // 3
        np.testing.assert_array_equal(v[2 * n:].view(np.uint16 if v.dtype == np.uint16 else np.uint32), b[k].view(np.uint16 if v.dtype == np.uint16 else np.uint32), err_msg=k)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def backward_reference(regime, B, p):
    P, x = ref.make_case(regime, B)
    seed, sites = SEEDS[1], SITES[1]
    masks = ref.make_masks(seed, sites, B, p)
    R = ref.forward(P, x, None, None, masks, p, grad=True)
    dn3 = np.random.default_rng(17).standard_normal((B, L, D)).astype(np.float32)
    return P, masks, seed, sites, R, dn3, ref.backward_part0(R, dn3)


def bwd_desc(be, ins, B, P, packed, p, seed, sites, **kw):
    return _abi.TokenBlockBwdDesc(B=B, packed=be.ptr(packed), drop_p=p, seed=seed, site_embed=sites[0], site_attn_out=sites[2], site_ffn_act=sites[3],
                                  site_ffn_out=sites[4], **kw)


@pytest.mark.parametrize("with_n2", [True, False], ids=["n2", "n2-from-r2"])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("regime", ["benign", "offset", "sharp", "sparse"])
def test_backward_part0_against_autograd(be, regime, p, with_n2):
    """the saved activations handed to the kernel are the reference's own (cast to fp32, mu and rs included): the forward kernel is not involved"""
    B = 2
    P, masks, seed, sites, R, dn3, G = backward_reference(regime, B, p)
    f32 = lambda k: R[k].detach().numpy().astype(np.float32)
    ins = Ins(be)
    packed, _ = pack_weights(be, ins, P, False)
    o = {"dr1": Out(be, B * L * D), "dctx": Out(be, B * L * HE), "partials": Out(be, int(be.lib.eegclip_token_block_bwd_workspace_floats(B)))}
    o.update({k: Out(be, B * 32768, planes=True) for k in ("df2p", "dg1p", "da1p")})
    S = {k: f32(k) for k in ("n2", "r2", "r1", "f1", "mu1", "rs1", "mu2", "rs2", "mu3", "rs3")}
    d = bwd_desc(be, ins, B, P, packed, p, seed, sites, dn3=ins.add("dn3", dn3), n2=ins.add("n2", S["n2"]) if with_n2 else None,
                 **{k: ins.add(k, S[k]) for k in S if k != "n2"}, **{k: ins.add(k, P[k]) for k in ("ln1_g", "ln2_g", "ln3_g")}, **{k: v.ptr for k, v in o.items()},
                 # (a stored n2 must be USED: re-evaluating it from r2 gives nearly the same numbers, so the bias that the re-evaluation would need is NaN here)
                 ln2_b=ins.add("ln2_b", np.full(D, np.nan, np.float32) if with_n2 else P["ln2_b"]))
    assert be.lib.eegclip_token_block_bwd(ctypes.byref(d), 0, be.stream) == 0
    be.sync()
    K = {k: v.read() for k, v in o.items()}
    ins.check()
    ck = Checker(f"[{be.name} bwd0 {regime} p={p} n2={with_n2}]")
    f64 = lambda a: np.asarray(a, np.float64)
    W = {k: f64(v) for k, v in P.items()}
    ksc = ref.drop_scale(p) if p > 0 else 1.0
    mk = (lambda nm: masks[nm] * ksc) if masks is not None else (lambda nm: 1.0)
    df2, fhi, flo = decode_planes(K["df2p"], B)
    dg1, ghi, glo = decode_planes(K["dg1p"], B, FF)
    da1, ahi, alo = decode_planes(K["da1p"], B)
    # dY operands carry no ones column: channels 250 .. 255 of a 250-wide tensor are zero in both planes (channel 255 included), dg1 has 256 real channels
    plane_properties(ck, "df2p", fhi, flo, D, ones=False)
    plane_properties(ck, "dg1p", ghi, glo, FF, ones=False)
    plane_properties(ck, "da1p", ahi, alo, D, ones=False)
    dr1 = K["dr1"].reshape(B, L, D)
    dctx = f64(K["dctx"]).reshape(B, L, HE)
    part = K["partials"].reshape(B, 6, 256)
    # -- da1 = dropout'(dr1): the planes are the split of the fp32 product, exactly
    ksc32 = np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)
    exp = dr1 * ksc32 if masks is None else np.where(masks["attn_out"], dr1 * ksc32, np.float32(0.0))
    eh, el = split(exp.reshape(-1, D))
    ck.equal("da1p = split(dropout'(dr1))", np.stack([ahi[:, :, :D], alo[:, :, :D]]), np.stack([eh.reshape(B, L, D), el.reshape(B, L, D)]))
    # -- dctx = da1 Wo from the decoded da1 planes
    ck.close("dctx", dctx, da1 @ W["wo"], ref.lin_bound(da1, W["wo"].T, None, ref.C_LIN_BWD))
    # -- final LayerNorm' and LayerNorm2' from the kernel's inputs; n2 re-evaluated in fp32 from r2 carries the forward LayerNorm's round-off
    n2_in = f64(S["n2"])
    dx_in = None
    if not with_n2:
        _, _, _, dx_in, _, _ = ref.ln_bounds(f64(S["r2"]), W["ln2_g"], W["ln2_b"])
        dx_in = dx_in + ref.U24 * np.abs(n2_in)                # (+ the rounding of the stored fp32 n2 this test's reference was built from)
    dn2, b3 = ref.ln_bwd_bounds(f64(dn3), n2_in, W["ln3_g"], dx_in=dx_in)
    dr2, b2 = ref.ln_bwd_bounds(dn2, f64(S["r2"]), W["ln2_g"], ddy=b3)
    ck.close("df2", df2, dr2 * mk("ffn_out"), (b2 + ref.PLANE * np.abs(dr2)) * mk("ffn_out"))
    # -- dg1 = dropout' gelu' (df2 W2) from the decoded df2 planes
    f1 = f64(S["f1"])
    gg = ref.gelu_grad(ref.t64(f1)).numpy() * mk("ffn_act")
    lin = df2 @ W["w2"]
    ck.close("dg1", dg1, lin * gg, ref.lin_bound(df2, W["w2"].T, None, ref.C_LIN_BWD) * np.abs(gg) + ref.C_GELU_GRAD * ref.U24 * (1 + np.abs(f1)) * np.abs(lin) * mk("ffn_act")
             + ref.PLANE * np.abs(lin * gg))
    # -- the final LayerNorm's parameter-gradient rows from the kernel's inputs
    _, _, _, xh3, rs3 = ref.ln_bwd_ref(f64(dn3), n2_in, W["ln3_g"])
    ady = np.abs(f64(dn3))
    dxh = ref.C_LN_BWD * ref.U24 * (rs3 * np.abs(n2_in).mean(-1, keepdims=True) + np.abs(xh3)) + (0.0 if dx_in is None else rs3 * dx_in)
    ck.close("partials g3", part[:, 0, :D], (f64(dn3) * xh3).sum(1), (ady * dxh).sum(1) + ref.C_LN_BWD * ref.U24 * (ady * np.abs(xh3)).sum(1))
    ck.close("partials b3", part[:, 1, :D], f64(dn3).sum(1), ref.C_LN_BWD * ref.U24 * ady.sum(1))
    # -- end to end against autograd
    got = {"df2": df2, "dg1": dg1, "da1": da1, "dr1": dr1, "dctx": dctx, "partials": part[:, :, :D]}
    for k, v in got.items():
        r = G[k].numpy()
        ck.close(k, v, r, e2e_tolerance(regime, k, r, plane=k in ("df2", "dg1", "da1")), kind="e2e")
    ck.done()


@pytest.mark.parametrize("with_dr1p", [True, False], ids=["dr1p", "no-dr1p"])
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("regime", ["benign", "offset"])
def test_backward_part1_against_autograd(be, regime, p, with_dr1p):
    B = 2
    P, masks, seed, sites, R, _, _ = backward_reference(regime, B, p)
    rng = np.random.default_rng(23)
    dqkv = (rng.standard_normal((B * L, 3 * HE)) * np.exp(rng.uniform(-3, 3, (1, 3 * HE)))).astype(np.float32)      # columns of very different magnitude
    dr1_in = rng.standard_normal((B, L, D)).astype(np.float32)
    ins = Ins(be)
    packed, _ = pack_weights(be, ins, P, False)
    groups = []
    for g in range(3):                                         # dq | dk | dv -> token planes, channel 64 head + d, groups B * 64 KB apart
        dst = be.dev(np.full(B * 32768, NAN_P, np.uint16))
        X = be.dev(np.ascontiguousarray(dqkv[:, g * HE:(g + 1) * HE]))
        assert be.lib.eegclip_tok_planes_from_f32(be.ptr(X), HE, B * L, HE, 1, 0, be.ptr(dst), be.stream) == 0
        be.sync()
        groups.append(be.host(dst))
    blob = np.concatenate(groups)
    seen = np.concatenate([decode_planes(g, B, HE, heads=True)[0] for g in groups], -1)      # what the kernel reads: hi + lo
    o = {"dr1": Out(be, B * L * D, init=dr1_in), "dr1p": Out(be, B * 32768, planes=True)}
    d = bwd_desc(be, ins, B, P, packed, p, seed, sites, dqkvp=ins.add("dqkvp", blob), dr1=o["dr1"].ptr, dr1p=o["dr1p"].ptr if with_dr1p else None)
    assert be.lib.eegclip_token_block_bwd(ctypes.byref(d), 1, be.stream) == 0
    be.sync()
    out = o["dr1"].read().reshape(B, L, D)
    pl = o["dr1p"].read(written=with_dr1p)
    ins.check()
    ck = Checker(f"[{be.name} bwd1 {regime} p={p}]")
    want = ref.backward_part1(R, seen, dr1_in).numpy()
    m = masks["embed"] * ref.drop_scale(p) if masks is not None else 1.0
    f64 = lambda a: np.asarray(a, np.float64)
    bound = m * (ref.lin_bound(seen, f64(P["wqkv"]).T, None, ref.C_LIN_BWD) + 2 * ref.U24 * (np.abs(f64(dr1_in)) + np.abs(want)))
    ck.close("dh", out, want, bound)
    if with_dr1p:
        _, hi, lo = decode_planes(pl, B)
        plane_properties(ck, "dr1p", hi, lo, D, ones=False)
        eh, el = split(out.reshape(-1, D))
        ck.equal("dr1p = split(dr1)", np.stack([hi[:, :, :D], lo[:, :, :D]]), np.stack([eh.reshape(B, L, D), el.reshape(B, L, D)]))
    ck.done()


@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_backward_part2_adds_the_column_sums(be, B):
    """dln*_g / dln*_b += the fp64 column sums of `partials` (B, 6, 256); the outputs are 250 floats between canaries, so columns 250 .. 255 cannot leak"""
    rng = np.random.default_rng(B)
    part = (rng.standard_normal((B, 6, 256)) * np.exp(rng.uniform(-2, 2, (1, 6, 256)))).astype(np.float32)
    part[:, :, D:] = 1e6                                       # would be visible anywhere
    pre = rng.standard_normal((6, D)).astype(np.float32) + 3.0
    ins = Ins(be)
    outs = [Out(be, D, init=pre[v]) for v in range(6)]
    dummy = be.dev(np.zeros(8, np.uint16))
    d = _abi.TokenBlockBwdDesc(B=B, packed=be.ptr(dummy), partials=ins.add("partials", part), drop_p=0.0,
                               **{k: outs[v].ptr for v, k in enumerate(("dln3_g", "dln3_b", "dln2_g", "dln2_b", "dln1_g", "dln1_b"))})
    assert be.lib.eegclip_token_block_bwd(ctypes.byref(d), 2, be.stream) == 0
    be.sync()
    got = np.stack([o.read() for o in outs])
    ins.check()
    p64 = part[:, :, :D].astype(np.float64)
    want = pre + p64.sum(0)
    # at most B + 1 fp32 additions per address (the per-slice sums, then one atomic add per slice), each rounding at most 2^-24 of the running magnitude
    bound = (B + 1) * ref.U24 * (np.abs(p64).sum(0) + np.abs(pre))
    ck = Checker(f"[{be.name} bwd2 B={B}]")
    ck.close("dln", got, want, bound)
    ck.done()


# ---- argument checks: refused before any launch -------------------------------------------------------------------------------------------
def _valid_descs(be):
    B = 1
    keep = []

    def buf(n, dt=np.float32):
        keep.append(be.dev(np.zeros(n + 8, dt)))
        return be.ptr(keep[-1])
    packed = buf(int(be.lib.eegclip_token_block_packed_bytes()) // 2, np.uint16)
    fw = dict(B=B, x=buf(NCH * T), packed=packed, bv=buf(D), pe=buf(NCH * D), tokens=buf(10 * D), drop_p=0.25, eps=ref.EPS, scale=ref.SCALE, seed=1,
              site_embed=0, site_attn=1, site_attn_out=2, site_ffn_act=3, site_ffn_out=4)
    fw.update({k: buf(3 * HE) for k in ("bqkv", "bo", "ln1_g", "ln1_b", "b1", "b2", "ln2_g", "ln2_b", "ln3_g", "ln3_b")})
    fw.update({k: buf(L * 3 * HE) for k in ("h", "qkv", "r1", "mu1", "rs1", "f1", "r2", "n2", "mu2", "rs2", "n3", "mu3", "rs3")})
    fw.update({k: buf(32768, np.uint16) for k in ("xp", "hp", "ctxp", "n1p", "g1p")})
    bw = dict(B=B, packed=packed, drop_p=0.25, seed=1, site_embed=0, site_attn_out=2, site_ffn_act=3, site_ffn_out=4)
    bw.update({k: buf(L * FF) for k in ("dn3", "n2", "r2", "r1", "f1", "mu1", "rs1", "mu2", "rs2", "mu3", "rs3", "ln1_g", "ln2_g", "ln2_b", "ln3_g", "dr1", "dctx")})
    bw["partials"] = buf(6 * 256)
    bw.update({k: buf(32768, np.uint16) for k in ("df2p", "dg1p", "da1p", "dr1p")})
    bw["dqkvp"] = buf(3 * 32768, np.uint16)
    bw.update({k: buf(D) for k in ("dln3_g", "dln3_b", "dln2_g", "dln2_b", "dln1_g", "dln1_b")})
    return fw, bw, keep, buf


def test_entry_points_refuse_bad_arguments(be):
    fw, bw, keep, buf = _valid_descs(be)
    fwd = lambda **kw: be.lib.eegclip_token_block_fwd(ctypes.byref(_abi.TokenBlockDesc(**{**fw, **kw})), be.stream)
    bwd = lambda part, **kw: be.lib.eegclip_token_block_bwd(ctypes.byref(_abi.TokenBlockBwdDesc(**{**bw, **kw})), part, be.stream)
    required = ["x", "packed", "bv", "pe", "tokens", "bqkv", "bo", "ln1_g", "ln1_b", "b1", "b2", "ln2_g", "ln2_b", "ln3_g", "ln3_b", "h", "qkv", "r1", "mu1", "rs1",
                "f1", "r2", "mu2", "rs2", "n3", "mu3", "rs3", "hp", "ctxp", "n1p", "g1p"]
    for k in required:
        assert fwd(**{k: None}) == EINVAL, k
    assert fwd(drop_p=1.0) == EINVAL and fwd(drop_p=-0.125) == EINVAL and fwd(B=0) == EINVAL
    assert fwd(cs_rows=buf(160, np.float64)) == EINVAL                                     # cs_rows without cs_w25
    subj = buf(4, np.int32)
    assert fwd(embed_subject=subj, packed_embed=fw["packed"], bv_stride=251) == EINVAL       # odd bv_stride
    assert fwd(embed_subject=subj, packed_embed=None, bv_stride=250) == EINVAL
    for k in ("h", "f1", "hp", "packed"):                                                    # a 16-byte buffer offset by 8
        assert fwd(**{k: fw[k] + 8}) == EALIGN, k
    assert fwd(r1=fw["r1"] + 4) == EALIGN                                                    # an 8-byte buffer offset by 4
    for part, names in ((0, ["packed", "dn3", "r2", "r1", "f1", "mu1", "rs1", "mu2", "rs2", "mu3", "rs3", "ln1_g", "ln2_g", "ln3_g", "df2p", "dg1p", "da1p", "dr1", "dctx",
                             "partials"]),
                        (1, ["packed", "dqkvp", "dr1"]), (2, ["packed", "partials", "dln3_g", "dln3_b", "dln2_g", "dln2_b", "dln1_g", "dln1_b"])):
        for k in names:
            assert bwd(part, **{k: None}) == EINVAL, (part, k)
        assert bwd(part, drop_p=1.0) == EINVAL and bwd(part, drop_p=-0.125) == EINVAL
    assert bwd(0, n2=None, ln2_b=None) == EINVAL                                            # n2 is re-evaluated from r2: that needs ln2_b
    assert bwd(3) == EINVAL and bwd(-1) == EINVAL
    assert bwd(0, f1=bw["f1"] + 8) == EALIGN and bwd(0, df2p=bw["df2p"] + 8) == EALIGN and bwd(0, dn3=bw["dn3"] + 4) == EALIGN
    assert bwd(1, dr1=bw["dr1"] + 8) == EALIGN and bwd(1, dqkvp=bw["dqkvp"] + 8) == EALIGN and bwd(1, dr1p=bw["dr1p"] + 8) == EALIGN
    be.sync()
