"""fp64 reference of the encoder's transformer block (csrc/token_block.hip), written from oracle/atms.py:98-136 and the header comment of
include/eegclip.h (eegclip_token_block_desc / _bwd_desc), NOT from the kernel: value embedding (one per subject in the joint model) + positional
table + subject token + dropout, q | k | v, 4-head softmax attention with probability dropout, output projection, dropout + residual + LayerNorm,
FFN 250 -> 256 (erf GELU, dropout) -> 250, dropout + residual + LayerNorm, final LayerNorm.  The backward is autograd on the same graph.

The same chain also runs as a MODEL of the kernels' arithmetic (fp32 everywhere, every Linear as split-bf16 products a_hi b_hi + a_hi b_lo + a_lo b_hi with fp32
accumulation): the model is never compared with the kernel, it only says how far such arithmetic may drift from fp64, which fixes the tolerances of
tests/test_kernels_token_block.py.  `python tests/token_block_ref.py` prints the measured constants recorded below.

Tolerances (derived here, checked against this reference alone on the CPU; measured figures beside each constant):

  Linear          |kernel - fp64(kernel's own input)| <= C_LIN 2^-16 (|x| |W|^T + |b|) elementwise.  Per product the relative error is a few 2^-18 (the dropped
                  a_lo b_lo term is <= 2^-18 |a b|, the residual of a two-term bf16 split <= 2^-17 |a|), fp32 accumulation of <= 256 terms adds ~2^-24 sqrt(K).
  LayerNorm       y: C_LN 2^-24 (|g| rs (mean|x| + |x - mu|) + |b| + |y|), mu: C_LN 2^-24 mean|x|, rs: C_LN 2^-24 rs -- the error of a two-pass fp32 evaluation
                  is the error of the mean (relative to the row's magnitude, NOT its spread: what the `offset` regime is about) plus a few roundings.
  GELU / GELU'    C_GELU 2^-24 (|x| + |gelu x|) and C_GELU 2^-24 (1 + |x|).
  softmax         a perturbation ds of the logits moves P_j to P_j exp(ds_j) / sum_k P_k exp(ds_k), within P_j exp(+-(ds_j + max ds)); ds = the Linear bound
                  of q k^T (times scale) + C_SM 2^-24 (|s| + |max| + 1) for the roundings of s, s - max, exp and the row sum; probabilities below the
                  smallest normal fp32 may flush to zero.
  token planes    |hi + lo - v| <= 2^-17 |v| (PLANE) on top of the bound of the fp32 value they split.
Each C is 4 x the worst ratio error / scale of the fp32 model against fp64 over the four regimes (MEASURED below).
"""
import math

import numpy as np
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file runs as a script)
from philox_np import keep_mask
from test_kernels_wgrad import bf16_round, head_channels, planes_to_f32, split  # noqa: F401  (re-exported: the plane decoder's pieces)

L, D, T, NCH, H, E, HE, FF = 64, 250, 250, 63, 4, 62, 248, 256
SITE_NAMES = ("embed", "attn", "attn_out", "ffn_act", "ffn_out")
MASK_SHAPES = {"embed": (L, D), "attn": (H, L, L), "attn_out": (L, D), "ffn_act": (L, FF), "ffn_out": (L, D)}      # per sample; flat index is batch-major
EPS = 1e-5
SCALE = 1.0 / math.sqrt(E)

# ---- measured on the CPU (python tests/token_block_ref.py): worst error / scale of the fp32 split-bf16 model against fp64 of its own stage input, over the
# regimes benign / offset / sharp / sparse at drop_p 0, 0.25, 0.9, B = 3.  The constants are 4 x these ratios.
MEASURED = {"lin": 0.963, "lin_bwd": 0.62, "ln": 2.962, "ln_bwd": 3.55, "gelu": 1.43, "gelu_grad": 1.238, "softmax": 0.139}
C_LIN = 4 * 0.963           # forward Linears: q | k | v, out projection, FFN 1, FFN 2 (worst ratio 0.963)
C_LIN_BWD = 4 * 0.62        # dg1 = df2 W2 (with dropout' gelu'), dctx = da1 Wo; also dn1 += df1 W1 and dh += d{q,k,v} W{q,k,v} (worst ratio 0.62)
C_LN = 4 * 2.962            # LayerNorm forward: y, mu, rs (worst ratio 2.962, the `offset` regime)
C_LN_BWD = 4 * 3.55         # LayerNorm backward dx (worst ratio 3.55)
C_GELU = 4 * 1.43           # (worst ratio 1.43)
C_GELU_GRAD = 4 * 1.238     # (worst ratio 1.238)
C_SM = 4.0                  # softmax: one rounding each of s, s - max, the row sum, the reciprocal, <= 2 ulp of exp -- by reasoning; the fp32 model
                            # reaches 0.139 / 4 = 0.035 of the whole attention bound (attention_bound): the 4 x margin holds with room
U16, U24 = 2.0 ** -16, 2.0 ** -24
PLANE = 2.0 ** -17          # |hi + lo - v| <= 2^-17 |v|: for v in [1, 2) the residual v - hi is at most 2^-8 (half a bf16 spacing), and rounding it to bf16
                            # leaves at most half of ITS spacing, 2^-17 (reached near powers of two; bf16 underflow is irrelevant at these magnitudes)

# ---- end to end: the drift of the fp32 split-bf16 model of the WHOLE chain from the fp64 chain, max |model - fp64| / max |fp64| per tensor, worst over the cases of
# a regime (B 1 and 3, drop_p 0 / 0.25 / 0.9, both seeds and site sets, with and without token ids and per-subject embeddings; the backward tensors: B = 2,
# drop_p 0 / 0.25).  This cannot be derived; the tests allow 4 x these figures.  (python tests/token_block_ref.py prints the table.)
E2E_DRIFT = {
    "benign": {'h': 4.22e-06, 'qkv': 7.06e-06, 'ctx': 0.000109, 'r1': 7.94e-05, 'n1': 0.000119, 'mu1': 5.59e-05, 'rs1': 8.66e-05, 'f1': 0.000156, 'g1': 0.000115, 'r2': 0.000107, 'n2': 0.000109, 'mu2': 8.71e-05, 'rs2': 3.31e-05, 'n3': 0.000109, 'mu3': 9.86e-05, 'rs3': 1.01e-05, 'df2': 1.86e-06, 'dg1': 1.45e-05, 'da1': 5.63e-06, 'dr1': 5.63e-06, 'dctx': 7.67e-06, 'partials': 9.32e-06},
    "offset": {'h': 1.71e-06, 'qkv': 9.23e-06, 'ctx': 0.000229, 'r1': 4.4e-05, 'n1': 9.39e-05, 'mu1': 6.22e-06, 'rs1': 1.74e-05, 'f1': 6.03e-05, 'g1': 6.03e-05, 'r2': 1.36e-06, 'n2': 4.16e-05, 'mu2': 1.83e-07, 'rs2': 2.97e-06, 'n3': 4.25e-05, 'mu3': 0.000278, 'rs3': 4.46e-06, 'df2': 1.9e-06, 'dg1': 3.4e-05, 'da1': 7.63e-06, 'dr1': 7.63e-06, 'dctx': 1.03e-05, 'partials': 1.03e-05},
    "sharp": {'h': 4.53e-06, 'qkv': 8.87e-06, 'ctx': 0.000737, 'r1': 0.000723, 'n1': 0.00136, 'mu1': 0.000644, 'rs1': 0.000702, 'f1': 0.00183, 'g1': 0.00209, 'r2': 0.00162, 'n2': 0.00152, 'mu2': 0.00064, 'rs2': 0.000376, 'n3': 0.00143, 'mu3': 0.000956, 'rs3': 3.83e-05, 'df2': 1.87e-05, 'dg1': 0.000221, 'da1': 0.0001, 'dr1': 0.0001, 'dctx': 0.0001, 'partials': 9.04e-05},
    "sparse": {'h': 4.64e-06, 'qkv': 8.06e-06, 'ctx': 8.5e-05, 'r1': 7.88e-05, 'n1': 0.000102, 'mu1': 3.14e-05, 'rs1': 4.83e-05, 'f1': 9.24e-05, 'g1': 7.89e-05, 'r2': 4.48e-05, 'n2': 5.49e-05, 'mu2': 5.85e-05, 'rs2': 2.63e-05, 'n3': 5.83e-05, 'mu3': 4.93e-05, 'rs3': 4.02e-06, 'df2': 1.55e-06, 'dg1': 1.07e-05, 'da1': 4.65e-06, 'dr1': 4.65e-06, 'dctx': 7.43e-06, 'partials': 7.7e-06},
}


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


# ------------------------------------------------------------------------------------------------------------------------------------------
# parameters and inputs of the four regimes
def make_case(regime, B, seed=0, n_subjects=0, bv_stride=D):
    """-> (P, x): P = dict of fp32 arrays in nn.Linear layout (wv (250,250) or (S,250,250), bv (250) or (S, bv_stride), pe (63,250), tokens (10,250),
    wqkv (744,250), bqkv, wo (250,248), bo, w1 (256,250), b1, w2 (250,256), b2, ln{1,2,3}_{g,b}), x (B,63,250).  Deterministic."""
    from eeg_image_decode_amd import synthetic as syn
    rng = np.random.default_rng([seed, {"benign": 1, "offset": 2, "sharp": 3, "sparse": 4}[regime]])
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = lambda o, i: (n(o, i) / np.float32(math.sqrt(i))).astype(np.float32)
    S = max(n_subjects, 1)
    P = {"wv": np.stack([w(D, T) for _ in range(S)]), "bv": 0.05 * n(S, D), "pe": syn.sinusoid_table(NCH, D), "tokens": n(10, D),
         "wqkv": w(3 * HE, D), "bqkv": 0.05 * n(3 * HE), "wo": w(D, HE), "bo": 0.05 * n(D), "w1": w(FF, D), "b1": 0.05 * n(FF), "w2": w(D, FF), "b2": 0.05 * n(D)}
    for k in ("ln1", "ln2", "ln3"):
        P[k + "_g"], P[k + "_b"] = 1.0 + 0.1 * n(D), 0.05 * n(D)
    x = n(B, NCH, T)
    if regime == "offset":
        for k, m in (("bv", S * D), ("bqkv", 3 * HE), ("bo", D), ("b1", FF), ("b2", D)):
            P[k] = n(m).reshape(P[k].shape)
        for k in ("ln1", "ln2", "ln3"):
            P[k + "_g"] = (np.exp(rng.uniform(math.log(0.25), math.log(4.0), D)) * np.where(rng.random(D) < 0.3, -1.0, 1.0)).astype(np.float32)
            P[k + "_b"] = (2.0 * n(D)).astype(np.float32)
        # rows whose mean dwarfs their spread.  A common offset in h itself (a scaled token row, a scaled bv) comes back out of q | k | v as a SPREAD (h W has
        # the row sums of W in it), so it cannot alone make r1 / r2 mean-dominated: the token row and bv are scaled (large, not small, inputs) and the
        # offsets that survive to the LayerNorms ride on the two biases that feed the residuals directly, bo -> r1 and b2 -> r2.
        P["tokens"][9] *= 8.0
        P["bv"] *= 3.0
        P["bo"] += 600.0
        P["b2"] += 900.0
    if regime == "sharp":
        # per head: scale Wq, bq so that the largest |logit| of rows 1.. (independent of the token row) in eval mode reaches 85 (head 0: 220, a few logits above
        # the fp32 overflow point of exp, 88.7)
        R = forward({**P, "wv": P["wv"][0], "bv": P["bv"][0]}, x, None, None, None, 0.0)
        q, k = R["qkv"].reshape(B, L, 3, H, E)[:, 1:, 0], R["qkv"].reshape(B, L, 3, H, E)[:, 1:, 1]
        s = torch.einsum("bihd,bjhd->bhij", q, k) * SCALE
        for hd in range(H):
            f = np.float32((220.0 if hd == 0 else 85.0) / float(s[:, hd].abs().max()))
            P["wqkv"][hd * E:(hd + 1) * E] *= f
            P["bqkv"][hd * E:(hd + 1) * E] *= f
    if regime == "sparse":
        x[0] = 0.0
        if B > 1:
            x[1, 1:62] = 0.0
    if n_subjects:
        bv = np.zeros((S, bv_stride), np.float32)
        bv[:, :D] = P["bv"]
        bv[:, D:] = np.nan                                     # the gap between two subjects' bias rows is never read into a result
        P["bv"] = bv
    else:
        P["wv"], P["bv"] = P["wv"][0], P["bv"][0]
    return P, x


def make_masks(seed, sites, B, p):
    """the five keep masks of a launch, batch-major flat element index (tests/test_model_gpu.py), or None at p = 0"""
    if p <= 0:
        return None
    return {nm: keep_mask(seed, int(site), B * int(np.prod(MASK_SHAPES[nm])), np.float32(p)).reshape((B,) + MASK_SHAPES[nm]) for nm, site in zip(SITE_NAMES, sites)}


# ------------------------------------------------------------------------------------------------------------------------------------------
# arithmetic: exact (fp64) or the model of the kernels' (fp32, split-bf16 products)
def _split_t(a):
    hi = a.bfloat16().float()
    return hi, (a - hi).bfloat16().float()


def x3mm(a, b):
    """a (.., M, K) @ b (K, N) as the three split-bf16 products with fp32 accumulation"""
    ah, al = _split_t(a)
    bh, bl = _split_t(b)
    return ah @ bh + ah @ bl + al @ bh


class _X3Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(w)
        return x3mm(x, w.t().contiguous()) + b

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        return x3mm(dy, w), None, None


class _X3Bmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return x3mm(a, b)

    @staticmethod
    def backward(ctx, dy):                                     # (the attention backward is another kernel: nothing compared here flows through it)
        a, b = ctx.saved_tensors
        return dy @ b.transpose(-1, -2), a.transpose(-1, -2) @ dy


class Arith:
    def __init__(self, model):
        self.model = model
        self.dt = torch.float32 if model else torch.float64

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(self.dt)

    def linear(self, x, w, b):
        return _X3Linear.apply(x, w, b) if self.model else x @ w.t() + b

    def bmm(self, a, b):
        return _X3Bmm.apply(a, b) if self.model else a @ b


def layer_norm(x, g, b, eps):
    """two-pass mean / biased variance; -> (y, mu, rs)"""
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    rs = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rs * g + b, mu[..., 0], rs[..., 0]


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def drop_scale(p):
    """1 / (1 - p) for the fp32 probability the descriptor carries"""
    return 1.0 / (1.0 - float(np.float32(p)))


def attention(A, qkv, mask, ksc, scale):
    """(B, 64, 744) -> ctx (B, 64, 248), P (B, 4, 64, 64) after dropout, logits"""
    B = qkv.shape[0]
    q, k, v = (qkv[..., i * HE:(i + 1) * HE].reshape(B, L, H, E).permute(0, 2, 1, 3) for i in range(3))
    s = A.bmm(q, k.transpose(-1, -2)) * scale
    Pm = torch.softmax(s, -1) if not A.model else _softmax32(s)
    Pd = Pm * (mask.to(Pm.dtype) * ksc) if mask is not None else Pm
    return A.bmm(Pd, v).permute(0, 2, 1, 3).reshape(B, L, HE), Pd, s


def _softmax32(s):
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e * (1.0 / e.sum(-1, keepdim=True))


def forward(P, x, ids, embed_subject, masks, drop_p, eps=EPS, scale=SCALE, model=False, grad=False):
    """Every tensor eegclip_token_block_fwd writes, as torch tensors of shape (B, 64, ..) (qkv (B, 64, 744) = q | k | v, column 62 head + d; mu / rs (B, 64)),
    plus the graph's leaves when grad=True.  masks: dict of the five boolean keep masks (make_masks) or None."""
    A = Arith(model)
    B = x.shape[0]
    W = {k: A.t(v) for k, v in P.items()}
    ksc = drop_scale(drop_p) if masks is not None else 1.0
    m = (lambda nm: None) if masks is None else (lambda nm: torch.from_numpy(masks[nm]))
    dr = lambda v, nm: v if masks is None else v * (m(nm).to(v.dtype) * ksc)
    xs = A.t(x)
    if embed_subject is None:
        e = A.linear(xs, W["wv"], W["bv"])
    else:
        e = torch.stack([A.linear(xs[i], W["wv"][int(s)], W["bv"][int(s), :D]) for i, s in enumerate(embed_subject)])
    e = e + W["pe"]
    tok = W["tokens"][torch.as_tensor(np.zeros(B, np.int64) if ids is None else np.asarray(ids, np.int64))]
    h0 = torch.cat([tok[:, None, :], e], 1)
    R = {}
    if grad:
        h0.requires_grad_(True)
        for k in ("ln1", "ln2", "ln3"):                        # one copy of the LayerNorm parameters per sample: their gradients are then the per-sample rows
            for s in "gb":
                W[k + "_" + s] = W[k + "_" + s].expand(B, 1, D).clone().requires_grad_(True)
                R[k + "_" + s] = W[k + "_" + s]
    R["h0"] = h0
    h = dr(h0, "embed")
    qkv = A.linear(h, W["wqkv"], W["bqkv"])
    ctx, Pd, s = attention(A, qkv, m("attn"), ksc, scale)
    a1 = A.linear(ctx, W["wo"], W["bo"])
    r1 = h + dr(a1, "attn_out")
    n1, mu1, rs1 = layer_norm(r1, W["ln1_g"], W["ln1_b"], eps)
    f1 = A.linear(n1, W["w1"], W["b1"])
    g1 = dr(gelu(f1), "ffn_act")
    f2 = A.linear(g1, W["w2"], W["b2"])
    r2 = n1 + dr(f2, "ffn_out")
    n2, mu2, rs2 = layer_norm(r2, W["ln2_g"], W["ln2_b"], eps)
    n3, mu3, rs3 = layer_norm(n2, W["ln3_g"], W["ln3_b"], eps)
    R.update(h=h, qkv=qkv, logits=s, ctx=ctx, a1=a1, r1=r1, n1=n1, mu1=mu1, rs1=rs1, f1=f1, g1=g1, f2=f2, r2=r2, n2=n2, mu2=mu2, rs2=rs2, n3=n3, mu3=mu3, rs3=rs3)
    if grad:
        for k in ("a1", "ctx", "r1", "f1", "f2", "qkv", "h"):
            R[k].retain_grad()
    return R


FWD_TENSORS = ("h", "qkv", "ctx", "r1", "n1", "mu1", "rs1", "f1", "g1", "r2", "n2", "mu2", "rs2", "n3", "mu3", "rs3")


def backward_part0(R, dn3):
    """autograd of a grad=True forward for the upstream gradient dn3 (B, 64, 250) -> df2, dg1 (= df1), da1, dr1, dctx (B, 64, ..) and the per-sample rows of the
    six LayerNorm parameter gradients, partials (B, 6, 250) in the kernel's order g3 b3 g2 b2 g1 b1"""
    for k in ("a1", "ctx", "r1", "f1", "f2", "ln1_g", "ln1_b", "ln2_g", "ln2_b", "ln3_g", "ln3_b"):
        R[k].grad = None
    R["n3"].backward(torch.as_tensor(dn3).to(R["n3"].dtype), retain_graph=True)
    out = {"df2": R["f2"].grad, "dg1": R["f1"].grad, "da1": R["a1"].grad, "dr1": R["r1"].grad, "dctx": R["ctx"].grad}
    out["partials"] = torch.stack([R[k].grad[:, 0] for k in ("ln3_g", "ln3_b", "ln2_g", "ln2_b", "ln1_g", "ln1_b")], 1)
    return {k: v.detach().clone() for k, v in out.items()}


def backward_part1(R, dqkv, dr1):
    """dropout'_embed(dr1 + dq Wq + dk Wk + dv Wv): the gradient of h0 when qkv receives dqkv (B, 64, 744) and h receives dr1 (B, 64, 250) directly"""
    dt = R["h0"].dtype
    (g,) = torch.autograd.grad([R["qkv"], R["h"]], [R["h0"]], [torch.as_tensor(dqkv).to(dt), torch.as_tensor(dr1).to(dt)], retain_graph=True)
    return g.detach()


# ------------------------------------------------------------------------------------------------------------------------------------------
# token planes
def decode_planes(blob, B, width=D, heads=False):
    """a token-plane tensor (B blocks [hi | lo][64][256] bf16) -> (value fp64 (B, 64, width) = hi + lo of the tensor's channels, hi, lo fp32 (B, 64, 256)).
    heads: the tensor's column 62 head + d is channel 64 head + d."""
    hi, lo = planes_to_f32(blob, B)
    ch = head_channels(width) if heads else np.arange(width)
    v = hi.astype(np.float64)[:, ch] + lo.astype(np.float64)[:, ch]
    return v.reshape(B, L, width), hi.reshape(B, L, 256), lo.reshape(B, L, 256)


# ------------------------------------------------------------------------------------------------------------------------------------------
# elementwise bounds (numpy fp64 in, fp64 out)
def lin_bound(x, w, b, c=C_LIN):
    return c * U16 * (np.abs(x) @ np.abs(w).T + (0.0 if b is None else np.abs(b)))


def ln_bounds(x, g, b, eps=EPS, c=C_LN):
    """-> (y, mu, rs, bound_y, bound_mu, bound_rs) of LayerNorm over the last axis in fp64"""
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    rs = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    y = d * rs * g + b
    ma = np.abs(x).mean(-1, keepdims=True)
    by = c * U24 * (np.abs(g) * rs * (ma + np.abs(d)) + np.abs(b) + np.abs(y))
    return y, mu[..., 0], rs[..., 0], by, c * U24 * ma[..., 0], c * U24 * rs[..., 0]


def ln_perturb(dx, xh, g, rs):
    """first-order bound of |d LayerNorm(x)| for an input perturbation bounded by dx (xh = (x - mu) rs, rs (.., 1))"""
    return np.abs(g) * rs * (dx + dx.mean(-1, keepdims=True) + np.abs(xh) * (np.abs(xh) * dx).mean(-1, keepdims=True))


def gelu_bound(x, y, c=C_GELU):
    return c * U24 * (np.abs(x) + np.abs(y))


def attention_bound(qkv, Pd, s, ksc, scale=SCALE):
    """bound of |ctx - fp64 ctx(qkv)| (B, 64, 248): logit perturbation -> probabilities -> P V, plus the P V products.  qkv, Pd (after dropout), s in fp64."""
    B = qkv.shape[0]
    q, k, v = (np.abs(qkv[..., i * HE:(i + 1) * HE]).reshape(B, L, H, E).transpose(0, 2, 1, 3) for i in range(3))
    ds = C_LIN * U16 * scale * (q @ k.transpose(0, 1, 3, 2)) + C_SM * U24 * (np.abs(s) + np.abs(s).max(-1, keepdims=True) + 1.0)
    # Pd = P mask ksc: the relative perturbation of a kept probability is that of P; the row term uses the undropped P <= sum over the kept / ksc, bounded
    # by the row's largest perturbation
    dP = Pd * np.expm1(ds + ds.max(-1, keepdims=True))         # (P'_j / P_j = exp(ds_j) / sum_k P_k exp(ds_k): no first-order assumption)
    dP = dP + ksc * 2.0 ** -126                                 # probabilities below the smallest normal fp32 may flush to zero
    return ((dP @ v) + C_LIN * U16 * (Pd @ v)).transpose(0, 2, 1, 3).reshape(B, L, HE)


# ------------------------------------------------------------------------------------------------------------------------------------------
def _measure():
    """prints the worst error / scale ratios of the fp32 split-bf16 model against fp64 behind MEASURED, and the end-to-end drift per regime and tensor"""
    worst = {k: 0.0 for k in MEASURED}
    up = lambda k, e, s: worst.__setitem__(k, max(worst[k], float(np.max(e / np.maximum(s, 1e-300)))))
    npf = lambda v: v.detach().double().numpy()
    for regime in ("benign", "offset", "sharp", "sparse"):
        for p in (0.0, 0.25, 0.9):
            B = 3
            P, x = make_case(regime, B)
            masks = make_masks(0x1234, (0, 1, 2, 3, 4), B, p)
            R = forward(P, x, None, None, masks, p, grad=True)
            M = forward(P, x, None, None, masks, p, model=True, grad=True)
            ksc = drop_scale(p) if p > 0 else 1.0
            P64 = {k: np.asarray(v, np.float64) for k, v in P.items()}
            # stage by stage: the model's stage output against fp64 of the MODEL's own stage input
            for xin, wk, bk, out in (("h", "wqkv", "bqkv", "qkv"), ("ctx", "wo", "bo", "a1"), ("n1", "w1", "b1", "f1"), ("g1", "w2", "b2", "f2")):
                xi = npf(M[xin])
                up("lin", np.abs(npf(M[out]) - (xi @ P64[wk].T + P64[bk])), lin_bound(xi, P64[wk], P64[bk], 1.0))
            for xin, k, outs in (("r1", "ln1", ("n1", "mu1", "rs1")), ("r2", "ln2", ("n2", "mu2", "rs2")), ("n2", "ln3", ("n3", "mu3", "rs3"))):
                y, mu, rs, by, bm, br = ln_bounds(npf(M[xin]), P64[k + "_g"], P64[k + "_b"], c=1.0)
                for ref, bd, o in ((y, by, outs[0]), (mu, bm, outs[1]), (rs, br, outs[2])):
                    up("ln", np.abs(npf(M[o]) - ref), bd)
            f1 = npf(M["f1"])
            gm = (masks["ffn_act"] * ksc) if masks else 1.0
            up("gelu", np.abs(npf(M["g1"]) - gelu(t64(f1)).numpy() * gm), gelu_bound(f1, gelu(t64(f1)).numpy(), 1.0) * gm + 1e-300)
            up("gelu_grad", np.abs(gelu_grad(torch.from_numpy(f1).float()).double().numpy() - gelu_grad(t64(f1)).numpy()), U24 * (1 + np.abs(f1)))
            qkv = npf(M["qkv"])
            cr, Pd, s = attention(Arith(False), t64(qkv), None if masks is None else torch.from_numpy(masks["attn"]), ksc, SCALE)
            up("softmax", np.abs(npf(M["ctx"]) - cr.numpy()), attention_bound(qkv, Pd.numpy(), s.numpy(), ksc) / 4.0)
            # backward GEMMs and LayerNorm backward: the model's autograd against fp64 autograd of the same graph (whole part 0 chain; the ratio is against
            # the Linear scale of the last GEMM of each output, a lower bound of the true scale)
            dn3 = np.random.default_rng(7).standard_normal((B, L, D))
            g64, g32 = backward_part0(R, dn3), backward_part0(M, dn3.astype(np.float32))
            e = {k: float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for k in g64}
            fw = {k: float((M[k].detach().double() - R[k].detach()).abs().max() / max(float(R[k].detach().abs().max()), 1e-300)) for k in FWD_TENSORS}
            print(f"{regime:7s} p={p:4.2f} end-to-end model drift / max|ref|: " + " ".join(f"{k}={v:.1e}" for k, v in {**fw, **e}.items()))
            da1 = npf(g32["da1"])
            up("lin_bwd", np.abs(npf(g32["dctx"]) - da1 @ P64["wo"]), lin_bound(da1, P64["wo"].T, None, 1.0))
            df2 = npf(g32["df2"])
            gg = gelu_grad(t64(npf(M["f1"]))).numpy() * gm
            up("lin_bwd", np.abs(npf(g32["dg1"]) - (df2 @ P64["w2"]) * gg), lin_bound(df2, P64["w2"].T, None, 1.0) * np.abs(gg) + C_GELU_GRAD * U24 * (1 + np.abs(f1)) * np.abs(df2 @ P64["w2"]) * np.abs(gm) + 1e-300)
            # LayerNorm backward alone (final LayerNorm): dn2 from dn3 in fp32 against fp64 on the model's n2
            n2 = npf(M["n2"])
            ref, bd = ln_bwd_bounds(dn3, n2, P64["ln3_g"], c=1.0)
            got = _ln_bwd32(dn3, n2, P64["ln3_g"])
            up("ln_bwd", np.abs(got - ref), bd)
    print({k: round(v, 3) for k, v in worst.items()})


def ln_bwd_ref(dy, x, g, eps=EPS):
    """fp64 LayerNorm backward: dx, and per-row-summed dgamma / dbeta over axis -2"""
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    rs = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    xh = d * rs
    gq = dy * g
    dx = rs * (gq - gq.mean(-1, keepdims=True) - xh * (gq * xh).mean(-1, keepdims=True))
    return dx, (dy * xh).sum(-2), dy.sum(-2), xh, rs


def ln_bwd_bounds(dy, x, g, eps=EPS, c=C_LN_BWD, dx_in=None, ddy=None):
    """-> (dx fp64, bound): dx = rs (gq - mean gq - xh mean(gq xh)), gq = dy g: the error of xh (that of the forward: relative to the row's magnitude) times
    |mean(gq xh)| and inside the second mean, plus roundings of each term.  dx_in / ddy: bounds of a perturbation of x (at fixed statistics) / of dy that the
    kernel's input carries against the x / dy given here (dx is linear in dy)."""
    dx, _, _, xh, rs = ln_bwd_ref(dy, x, g, eps)
    mean = lambda v: v.mean(-1, keepdims=True)
    gq, axh = np.abs(dy * g), np.abs(xh)
    dxh = c * U24 * (rs * mean(np.abs(x)) + axh) + (0.0 if dx_in is None else rs * dx_in)
    bound = c * U24 * rs * (gq + mean(gq) + axh * mean(gq * axh)) + rs * (dxh * np.abs(mean(dy * g * xh)) + axh * mean(gq * dxh))
    if ddy is not None:
        gd = np.abs(g) * ddy
        bound = bound + rs * (gd + mean(gd) + axh * mean(axh * gd))
    return dx, bound


def _ln_bwd32(dy, x, g, eps=EPS):
    dy, x, g = (torch.from_numpy(np.asarray(v, np.float32)) for v in (dy, x, g))
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    rs = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + np.float32(eps))
    xh = d * rs
    gq = dy * g
    return (rs * (gq - gq.mean(-1, keepdim=True) - xh * (gq * xh).mean(-1, keepdim=True))).double().numpy()


def _measure_e2e():
    table = {}
    for regime in ("benign", "offset", "sharp", "sparse"):
        worst = {}
        rel = lambda m, r: float((m.detach().double() - r.detach()).abs().max() / max(float(r.detach().abs().max()), 1e-300))
        for B in (1, 3):
            for p in (0.0, 0.25, 0.9):
                for v, (ids, subj, stride) in enumerate(((None, None, 0), ([9, 0, 9][:B], [2, 0, 2][:B], D))):
                    P, x = make_case(regime, B, n_subjects=3 if subj else 0, bv_stride=stride or D)
                    masks = make_masks((0x2A, 0x9E3779B97F4A7C15)[v], ((0, 1, 2, 3, 4), (11, 3, 200, 7, 5))[v], B, p)
                    R, M = forward(P, x, ids, subj, masks, p), forward(P, x, ids, subj, masks, p, model=True)
                    for k in FWD_TENSORS:
                        worst[k] = max(worst.get(k, 0.0), rel(M[k], R[k]))
        for p in (0.0, 0.25):
            B = 2
            P, x = make_case(regime, B)
            masks = make_masks(0x9E3779B97F4A7C15, (11, 3, 200, 7, 5), B, p)
            R, M = forward(P, x, None, None, masks, p, grad=True), forward(P, x, None, None, masks, p, model=True, grad=True)
            dn3 = np.random.default_rng(17).standard_normal((B, L, D)).astype(np.float32)
            g64, g32 = backward_part0(R, dn3), backward_part0(M, dn3)
            for k in g64:
                worst[k] = max(worst.get(k, 0.0), rel(g32[k], g64[k]))
        table[regime] = {k: float(f"{v:.2e}") for k, v in worst.items()}
    print("E2E_DRIFT = {")
    for r, t in table.items():
        print(f'    "{r}": {t},')
    print("}")


if __name__ == "__main__":
    _measure()
    _measure_e2e()
