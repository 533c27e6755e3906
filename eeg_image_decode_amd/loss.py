"""CLIP-symmetric InfoNCE with the reference's constructor and call signature (models/loss.py:78-141) on HIP kernels.

    loss = ClipLoss(local_loss=False, gather_with_grad=False, cache_labels=False, rank=0, world_size=1)(z_eeg, z_tgt, logit_scale)

`logit_scale` multiplies the logits RAW (no exp) exactly like the reference.  The N x N
logits are never written on the forward: csrc/infonce_fused.hip forms logits tiles on the bf16 matrix cores (split-bf16 products,
fp32 accumulate: logits within ~5e-5 of exact fp32 products) and keeps only per-row log-sum-exp partials; the backward recomputes
the tiles, writes the gradient matrix G once and the feature gradients are GEMMs over it.  Shapes the fused kernels do not take
(n, N or D not a multiple of 64) use the fp32-MFMA GEMM + row/column log-sum-exp kernels of csrc/loss.hip.  Gradients w.r.t. both
feature matrices and the scale are computed in the forward pass and handed to autograd.  world_size > 1 reproduces the three gather
modes of models/loss.py:20-75 over torch.distributed (RCCL on ROCm): all-gather forward, reduce-scatter of the gathered-feature
gradients when gather_with_grad is set.
"""
import ctypes
import os

import torch
import torch.nn as nn

from . import _abi
from ._lib import check, lib, raw_stream, require_cuda

D = _abi.dim


def _stream():
    return raw_stream()


def _gemm(M, N, K, A, Am, Ak, B, Bk, Bn, C, Cm, Cn, alpha=1.0, accumulate=0, split_k=1, precision=0):
    d = _abi.GemmDesc(M=M, N=N, K=K, A=A, Am=Am, Ak=Ak, B=B, Bk=Bk, Bn=Bn, C=C, Cm=Cm, Cn=Cn, Cpre=None, bias_n=None, bias_m=None,
                      R=None, Rm=D(0), Rn=D(0), alpha=alpha, accumulate=accumulate, act=0, drop_p=0.0, seed=0, drop_site=0, split_k=split_k,
                      precision=precision)
    check(lib().eegclip_gemm_f32(ctypes.byref(d), _stream()), "gemm")


def fused_enabled(n, N, Dm):
    """the fused kernels take whole 64-tiles (every training configuration of the path: 256 per GPU, D = 1024); EEGCLIP_INFONCE_FUSED=0 pins
    the GEMM + log-sum-exp route (diagnosis)"""
    return os.environ.get("EEGCLIP_INFONCE_FUSED", "1") != "0" and bool(lib().eegclip_infonce_fused_supported(int(n), int(N), int(Dm)))


def split_planes(x, planes):
    """fp32 features -> bf16 planes (hi, lo): x ~ hi + lo; lo is None in the one-product (throughput) mode"""
    n, Dm = x.shape
    hi = torch.empty(n, Dm, dtype=torch.bfloat16, device=x.device)
    lo = torch.empty(n, Dm, dtype=torch.bfloat16, device=x.device) if planes == 2 else None
    check(lib().eegclip_split_bf16(x.data_ptr(), hi.data_ptr(), lo.data_ptr() if lo is not None else None, n * Dm, _stream()), "split_bf16")
    return hi, lo


def split_planes_many(xs, planes, stack=None):
    """split_planes of several same-shaped feature matrices in ONE launch (eegclip_split_rows over a table: the query features and both
    targets of the batch loop -- three 5-us launches of a 1 MB split each, between the encoder's forward and the loss, became one).
    stack = a ((len(xs) - 1) n, D) fp32 tensor: the same launch also leaves xs[1:] stacked in it (the targets as ONE contraction operand of the
    query gradient, _grad_rows_stacked)"""
    # (only where launches, not bytes, are the cost: the table kernel converts element by element, the single-tensor one in 16-byte vectors --
    #  at N = 2048 three vectorised launches are faster: 82.6 vs 92.4 us for the whole loss forward)
    if (len(xs) == 1 or any(x.shape != xs[0].shape or not x.is_contiguous() for x in xs) or xs[0].shape[1] % 64 != 0 or len(xs) > 24
            or xs[0].numel() > (1 << 19)):
        if stack is not None:
            torch.cat(list(xs[1:]), out=stack)
        return [split_planes(x, planes) for x in xs]
    n, Dm = xs[0].shape
    buf = torch.empty(len(xs), 2, n, Dm, dtype=torch.bfloat16, device=xs[0].device)
    items = (_abi.SplitItem * len(xs))()
    for i, x in enumerate(xs):
        items[i] = _abi.SplitItem(src=x.data_ptr(), hi=buf[i, 0].data_ptr(), lo=buf[i, 1].data_ptr(), rows=n, cols=Dm, ld_src=Dm, ld_out=Dm, transpose=0,
                                  copy=stack[(i - 1) * n].data_ptr() if stack is not None and i > 0 else None, ld_copy=Dm)
    check(lib().eegclip_split_rows(items, len(xs), _stream()), "split_rows")
    return [(buf[i, 0], buf[i, 1] if planes == 2 else None) for i in range(len(xs))]


MAX_BLOCKS_PER_LAUNCH = 8          # IF_MAX_PROB of csrc/infonce_fused.hip (eegclip_infonce_fused_{fwd,grad} reject more)


def head_gemm_enabled(n, K, Dm):
    """the query gradient dA = [G_1 | .. | G_T] [B_1; ..; B_T] on the K-parallel plane GEMM (csrc/head_gemm.hip, round 6): gradient matrices as planes
    straight from the InfoNCE gradient pass, the stacked target planes read k-major (no transposed copy); other shapes keep the fp32-operand GEMM"""
    return n % 4 == 0 and K % 32 == 0 and Dm % 8 == 0


def stacked_target_planes(a_, bs, planes):
    """ONE split launch for the query features and the T targets: (ap, [bp_t], tp, aq) -- tp = the targets' planes STACKED, (2, T n, D): hi | lo of [B_1; ..; B_T],
    the k-major B operand of the query-gradient GEMM as it is (bp_t are its row blocks); aq = the query planes as one (2, n, D) tensor"""
    n, Dm = a_.shape
    T_ = len(bs)
    dev = a_.device
    aq = torch.empty(2, n, Dm, dtype=torch.bfloat16, device=dev)
    tp = torch.empty(2, T_ * n, Dm, dtype=torch.bfloat16, device=dev)
    items = (_abi.SplitItem * (T_ + 1))()
    items[0] = _abi.SplitItem(src=a_.data_ptr(), hi=aq[0].data_ptr(), lo=aq[1].data_ptr(), rows=n, cols=Dm, ld_src=Dm, ld_out=Dm, transpose=0)
    for t, b_ in enumerate(bs):
        items[1 + t] = _abi.SplitItem(src=b_.data_ptr(), hi=tp[0, t * n:].data_ptr(), lo=tp[1, t * n:].data_ptr(), rows=n, cols=Dm, ld_src=Dm, ld_out=Dm, transpose=0)
    check(lib().eegclip_split_rows(items, T_ + 1, _stream()), "split_rows")
    pick = (lambda hi, lo: (hi, lo if planes == 2 else None))
    return pick(aq[0], aq[1]), [pick(tp[0, t * n:(t + 1) * n], tp[1, t * n:(t + 1) * n]) for t in range(T_)], tp, aq


def query_grad_slabs(Gp, tp, n, K, Dm, slabs=None):
    """the K-parallel GEMM itself: (slabs (S, n, D) fp32, S).  Gp = [G_1 | .. | G_T] as planes (2, n, K), tp = the stacked target planes (2, K, D) read k-major.
    dA = slabs[0] + slabs[1] + .. in slice order -- added by whoever consumes it (the encoder's backward plan takes the slabs as they are; add_slabs for a
    plain tensor)"""
    L = lib()
    S = int(L.eegclip_head_gemm_slices(n, Dm, K))
    if slabs is None:
        slabs = torch.empty(S, n, Dm, dtype=torch.float32, device=Gp.device)
    d = _abi.HeadGemmDesc(a_hi=Gp[0].data_ptr(), a_lo=Gp[1].data_ptr(), b_hi=tp[0].data_ptr(), b_lo=tp[1].data_ptr(), lda=K, ldb=Dm, M=n, N=Dm, K=K,
                          slices=S, slab_stride=n * Dm, C=slabs.data_ptr(), ldc=Dm, b_kmajor=1)
    check(L.eegclip_head_gemm(ctypes.byref(d), _stream()), "head_gemm")
    return slabs, S


def infonce_small_enabled(n, T_, planes):
    """one process at the training batch size: logits as ONE K-parallel plane GEMM + two row-block kernels (csrc/infonce_small.hip, round 6) instead of the
    tile kernels' 64 workgroups that each walk D alone"""
    return planes == 2 and bool(lib().eegclip_infonce_small_supported(int(n), int(T_)))


def infonce_small(aq, tp, n, T_, Dm, weights, sc, acc, Gp):
    """loss / d scale added to acc[0] / acc[1]; G = [G_1 | .. | G_T] as planes into Gp (2, n, T n).  aq: query planes (2, n, D), tp: stacked target planes (2, T n, D)"""
    L, st = lib(), _stream()
    NC = T_ * n
    S = min(8, int(L.eegclip_head_gemm_slices(n, NC, Dm)))            # (eegclip_infonce_small_fwd adds at most 8 slabs)
    slabs = torch.empty(S, n, NC, dtype=torch.float32, device=aq.device)
    d = _abi.HeadGemmDesc(a_hi=aq[0].data_ptr(), a_lo=aq[1].data_ptr(), b_hi=tp[0].data_ptr(), b_lo=tp[1].data_ptr(), lda=Dm, ldb=Dm, M=n, N=NC, K=Dm, slices=S,
                          slab_stride=n * NC, C=slabs.data_ptr(), ldc=NC)
    check(L.eegclip_head_gemm(ctypes.byref(d), st), "head_gemm")
    ws = torch.empty(int(L.eegclip_infonce_small_workspace_floats(n, T_)), dtype=torch.float32, device=aq.device)
    check(L.eegclip_infonce_small_fwd(slabs.data_ptr(), S, n * NC, n, T_, sc.data_ptr(), ws.data_ptr(), st), "infonce_small_fwd")
    w4 = [float(w) for w in weights] + [0.0] * (4 - T_)
    check(L.eegclip_infonce_small_grad(n, T_, sc.data_ptr(), ws.data_ptr(), *w4, Gp[0].data_ptr(), Gp[1].data_ptr(), NC, acc.data_ptr(), acc.data_ptr() + 4, st),
          "infonce_small_grad")
    Gp._eegclip_keep = (slabs, ws)


def add_slabs(slabs):
    """slabs[0] + slabs[1] + .. in that order (what the slab-consuming kernels compute, bit for bit) -- ONE launch: eegclip_head_act's `pre` output is the slab
    sum (no bias, the activation output not requested); S - 1 torch adds were S - 1 launches and allocations on the host path of the row-sharded loss"""
    S = slabs.shape[0]
    if S == 1:
        return slabs[0]
    M, N = slabs.shape[1], slabs.shape[2]
    if slabs.is_contiguous() and N % 4 == 0 and S <= 16:
        out = torch.empty(M, N, dtype=torch.float32, device=slabs.device)
        check(lib().eegclip_head_act(slabs.data_ptr(), S, M * N, None, out.data_ptr(), None, None, None, M, N, _stream()), "head_act (slab sum)")
        out._eegclip_keep = slabs
        return out
    out = slabs[0]
    for i in range(1, S):
        out = out + slabs[i]
    return out


def fused_infonce(blocks, n, N, Dm, planes, n_total, sc, acc, want_grad, G_out=None, G_planes=None):
    """blocks = [(q planes, k planes, col0, weight)]: adds sum_blocks weight / n_total * sum_rows (lse_row - positive) to acc[0].
    want_grad = [(block index, index of the block whose lse is the second (per-key) normaliser, or None)]: for each, the gradient matrix
    G = s * dL/dS of that block ((n, N) fp32, written once) is returned and d loss / d s is added to acc[1].  G_out = where to write them (one (n, N)
    view per entry of want_grad, unit column stride, row stride a multiple of 4: e.g. side by side in one (n, T N) matrix).  G_planes = [(hi, lo)] bf16
    views of the same shape / strides: G leaves as the planes of the query-gradient GEMM instead (nothing is returned then)."""
    L = lib()
    dev = sc.device
    nb = len(blocks)
    ws = int(L.eegclip_infonce_fused_workspace_floats(n, N))
    buf = torch.empty(nb * (ws + 2 * n), dtype=torch.float32, device=dev)
    base = buf.data_ptr()
    arr = (_abi.InfonceProblem * nb)()
    for i, ((qh, ql), (kh, kl), col0, w) in enumerate(blocks):
        o = base + 4 * i * (ws + 2 * n)
        arr[i] = _abi.InfonceProblem(q_hi=qh.data_ptr(), q_lo=ql.data_ptr() if ql is not None else None, k_hi=kh.data_ptr(),
                                     k_lo=kl.data_ptr() if kl is not None else None, col0=int(col0), weight=float(w), part=o, diag=o + 4 * ws,
                                     lse=o + 4 * (ws + n), lse_k=None, G=None, ldg=0)
    st = _stream()
    # training (every block is differentiated: want_grad pairs each block with its swapped block): the forward leaves only the per-tile partials and the
    # gradient pass forms the log-sum-exps itself -- no finalize launch between the two tile launches (eegclip_infonce_fused_grad_finalize)
    covered = sorted(i for pair in want_grad for i in pair if i is not None)
    inline = (n == N and bool(want_grad) and covered == list(range(nb)) and all(ki is not None for _, ki in want_grad)
              and all(blocks[bi][3] == blocks[ki][3] for bi, ki in want_grad))
    for c0 in range(0, nb, MAX_BLOCKS_PER_LAUNCH):                  # (any number of targets: the launch table holds 8 blocks)
        chunk = (_abi.InfonceProblem * min(MAX_BLOCKS_PER_LAUNCH, nb - c0))(*arr[c0:c0 + MAX_BLOCKS_PER_LAUNCH])
        check(L.eegclip_infonce_fused_fwd(chunk, len(chunk), n, N, Dm, planes, n_total, sc.data_ptr(), None if inline else acc.data_ptr(), st),
              "infonce_fused_fwd")
    if not want_grad:
        return []
    garr = (_abi.InfonceProblem * len(want_grad))()
    Gs = []
    for j, (bi, ki) in enumerate(want_grad):
        garr[j] = arr[bi]
        if G_planes is not None:
            hi, lo = G_planes[j]
            garr[j].G, garr[j].ldg, garr[j].G_hi, garr[j].G_lo = None, hi.stride(0), hi.data_ptr(), lo.data_ptr()
        else:
            G = G_out[j] if G_out is not None else torch.empty(n, N, dtype=torch.float32, device=dev)
            Gs.append(G)
            garr[j].G, garr[j].ldg = G.data_ptr(), G.stride(0)
        garr[j].lse_k = arr[ki].lse if ki is not None else None
        if inline:
            garr[j].part_k, garr[j].diag_k = arr[ki].part, arr[ki].diag
    for c0 in range(0, len(want_grad), MAX_BLOCKS_PER_LAUNCH):
        chunk = (_abi.InfonceProblem * min(MAX_BLOCKS_PER_LAUNCH, len(want_grad) - c0))(*garr[c0:c0 + MAX_BLOCKS_PER_LAUNCH])
        if inline:
            check(L.eegclip_infonce_fused_grad_finalize(chunk, len(chunk), n, N, Dm, planes, n_total, sc.data_ptr(), acc.data_ptr(), acc.data_ptr() + 4, st),
                  "infonce_fused_grad_finalize")
        else:
            check(L.eegclip_infonce_fused_grad(chunk, len(chunk), n, N, Dm, planes, n_total, sc.data_ptr(), acc.data_ptr() + 4, st), "infonce_fused_grad")
    if Gs:
        Gs[0]._eegclip_keep = buf                  # the lse vectors must outlive the launch (stream-ordered allocator: already safe; explicit)
    return Gs


def _scale_ptr(logit_scale, device):
    if torch.is_tensor(logit_scale):
        s = logit_scale.detach()
        if s.device != device or s.dtype != torch.float32:
            s = s.to(device=device, dtype=torch.float32)
        return s.reshape(1).contiguous()
    return torch.full((1,), float(logit_scale), dtype=torch.float32, device=device)


def _logits_bf16(a_rows, b_cols, X):
    """raw logits a b^T on the bf16 matrix cores (features rounded to bf16 once, fp32 accumulate, fp32 out)"""
    L = lib()
    st = _stream()
    n, Dm = a_rows.shape
    N = b_cols.shape[0]
    a16 = torch.empty(n, Dm, dtype=torch.bfloat16, device=a_rows.device)
    b16 = torch.empty(N, Dm, dtype=torch.bfloat16, device=a_rows.device)
    check(L.eegclip_cast_bf16(a_rows.data_ptr(), a16.data_ptr(), n * Dm, st), "cast_bf16")
    check(L.eegclip_cast_bf16(b_cols.data_ptr(), b16.data_ptr(), N * Dm, st), "cast_bf16")
    check(L.eegclip_logits_bf16(a16.data_ptr(), b16.data_ptr(), X.data_ptr(), n, N, Dm, N, None, st), "logits_bf16")


def infonce_block(a_rows, b_cols, sc, col0, n_total, weight, row_term, col_term, need_grad, acc=None, bf16_logits=False):
    """One (n x N) logits block: loss contribution and, if need_grad, X <- weight * s*G in place.
    `acc` (2 floats: loss, dscale) is accumulated into when given.  Returns (loss[1], dscale[1], X or None)."""
    L = lib()
    n, Dm = a_rows.shape
    N = b_cols.shape[0]
    dev = a_rows.device
    X = torch.empty(n, N, dtype=torch.float32, device=dev)
    if bf16_logits and n % 128 == 0 and N % 128 == 0 and Dm % 64 == 0:
        _logits_bf16(a_rows, b_cols, X)
    else:
        _gemm(n, N, Dm, a_rows.data_ptr(), D(Dm), D(1), b_cols.data_ptr(), D(1), D(Dm), X.data_ptr(), D(N), D(1))
    st = _stream()
    lse = torch.empty(n + N, dtype=torch.float32, device=dev)
    lr, lc = lse[:n], lse[n:]
    if row_term:
        check(L.eegclip_lse_rows(X.data_ptr(), n, N, N, sc.data_ptr(), lr.data_ptr(), st), "lse_rows")
    if col_term:
        check(L.eegclip_lse_cols(X.data_ptr(), n, N, N, sc.data_ptr(), lc.data_ptr(), st), "lse_cols")
    if acc is None:
        acc = torch.zeros(2, dtype=torch.float32, device=dev)
    if need_grad or not (row_term and col_term and n == N):
        check(L.eegclip_infonce_grad(X.data_ptr(), n, N, N, col0, n_total, sc.data_ptr(), lr.data_ptr() if row_term else None,
                                     lc.data_ptr() if col_term else None, weight, acc.data_ptr(), acc.data_ptr() + 4, st), "infonce_grad")
    else:
        check(L.eegclip_infonce_loss(X.data_ptr(), n, N, sc.data_ptr(), lr.data_ptr(), lc.data_ptr(), weight, acc.data_ptr(), st), "infonce_loss")
        X = None
    return acc[0:1], acc[1:2], X


def _grad_rows(X, b_cols, out=None, precision=0):
    """dA (+)= (s G) B  -> (n, D)"""
    n, N = X.shape
    Dm = b_cols.shape[1]
    accumulate = out is not None
    if out is None:
        out = torch.empty(n, Dm, dtype=torch.float32, device=X.device)
    _gemm(n, Dm, N, X.data_ptr(), D(X.stride(0)), D(1), b_cols.data_ptr(), D(Dm), D(1), out.data_ptr(), D(Dm), D(1), accumulate=int(accumulate),
          precision=precision)
    return out


def _grad_cols(X, a_rows, out=None, precision=0):
    """dB (+)= (s G)^T A -> (N, D)"""
    n, N = X.shape
    Dm = a_rows.shape[1]
    accumulate = out is not None
    if out is None:
        out = torch.empty(N, Dm, dtype=torch.float32, device=X.device)
    _gemm(N, Dm, n, X.data_ptr(), D(1), D(X.stride(0)), a_rows.data_ptr(), D(Dm), D(1), out.data_ptr(), D(Dm), D(1), accumulate=int(accumulate),
          precision=precision)
    return out


def _sharded_blocks_on_planes(rank, W, a_, bs, a_all, b_alls, weights, sc, acc, planes):
    """sharded_blocks for the training configuration -- local_loss + gather_with_grad, frozen targets -- with every operand of the gradient GEMMs a bf16
    hi | lo plane (round 6; VERDICT r4 #7 / r5 #7: the fp32 gradient matrices, four fp32-operand GEMMs and the torch adds between them were ~180 us per
    rank at n = 256, N = 2048).  ONE split launch (gathered queries, gathered targets stacked, the rank's targets stacked), the forward over the 2 T
    blocks, two gradient launches -- G1_t = d loss / d S of (A_r, B_all,t) as planes (n, T N), and the swapped blocks' gradient matrices produced TRANSPOSED by
    the key-normalised form of the kernel, (N, T n) -- then da = [G1_1 | ..] [B_all,1; ..] (K-parallel plane GEMM, K = T N) and the gathered-copy gradient
    ga = [G2_1^T | ..] [B_r,1; ..] (K = T n).  Returns (da, ga)."""
    L, st, dev = lib(), _stream(), a_.device
    n, Dm = a_.shape
    N, T_ = W * n, len(bs)
    bf = torch.bfloat16
    qa = torch.empty(2, N, Dm, dtype=bf, device=dev)                  # gathered queries
    tall = torch.empty(2, T_ * N, Dm, dtype=bf, device=dev)            # [B_all,1; B_all,2; ..]
    tloc = torch.empty(2, T_ * n, Dm, dtype=bf, device=dev)            # [B_r,1; B_r,2; ..]
    items = (_abi.SplitItem * (1 + 2 * T_))()
    items[0] = _abi.SplitItem(src=a_all.data_ptr(), hi=qa[0].data_ptr(), lo=qa[1].data_ptr(), rows=N, cols=Dm, ld_src=Dm, ld_out=Dm, transpose=0)
    for t in range(T_):
        items[1 + t] = _abi.SplitItem(src=b_alls[t].data_ptr(), hi=tall[0, t * N:].data_ptr(), lo=tall[1, t * N:].data_ptr(), rows=N, cols=Dm, ld_src=Dm, ld_out=Dm,
                                      transpose=0)
        items[1 + T_ + t] = _abi.SplitItem(src=bs[t].data_ptr(), hi=tloc[0, t * n:].data_ptr(), lo=tloc[1, t * n:].data_ptr(), rows=n, cols=Dm, ld_src=Dm, ld_out=Dm,
                                           transpose=0)
    check(L.eegclip_split_rows(items, 1 + 2 * T_, st), "split_rows")
    lo = (lambda t_: t_.data_ptr()) if planes == 2 else (lambda t_: None)
    ws = int(L.eegclip_infonce_fused_workspace_floats(n, N))
    buf = torch.empty(2 * T_ * (ws + 2 * n), dtype=torch.float32, device=dev)
    arr = (_abi.InfonceProblem * (2 * T_))()
    for t, w in enumerate(weights):
        for j in range(2):
            o = buf.data_ptr() + 4 * (2 * t + j) * (ws + 2 * n)
            q = (qa[0, rank * n:], qa[1, rank * n:]) if j == 0 else (tloc[0, t * n:], tloc[1, t * n:])
            k = (tall[0, t * N:], tall[1, t * N:]) if j == 0 else (qa[0], qa[1])
            arr[2 * t + j] = _abi.InfonceProblem(q_hi=q[0].data_ptr(), q_lo=lo(q[1]), k_hi=k[0].data_ptr(), k_lo=lo(k[1]), col0=rank * n, weight=0.5 * float(w),
                                                 part=o, diag=o + 4 * ws, lse=o + 4 * (ws + n), lse_k=None, G=None, ldg=0)
    check(L.eegclip_infonce_fused_fwd(arr, 2 * T_, n, N, Dm, planes, n, sc.data_ptr(), acc.data_ptr(), st), "infonce_fused_fwd")
    g1 = torch.empty(2, n, T_ * N, dtype=bf, device=dev)
    g2t = torch.empty(2, N, T_ * n, dtype=bf, device=dev)
    ga_, gb_ = (_abi.InfonceProblem * T_)(), (_abi.InfonceProblem * T_)()
    for t, w in enumerate(weights):
        ga_[t] = arr[2 * t]
        ga_[t].G, ga_[t].ldg, ga_[t].G_hi, ga_[t].G_lo = None, T_ * N, g1[0, :, t * N:].data_ptr(), g1[1, :, t * N:].data_ptr()
        # the swapped block transposed: rows = the gathered queries, keys = the rank's targets of t; positive of query row i at key i - rank n
        gb_[t] = _abi.InfonceProblem(q_hi=qa[0].data_ptr(), q_lo=lo(qa[1]), k_hi=tloc[0, t * n:].data_ptr(), k_lo=lo(tloc[1, t * n:]), col0=-rank * n,
                                     weight=0.5 * float(w), part=None, diag=None, lse=None, lse_k=arr[2 * t + 1].lse, G=None, ldg=T_ * n,
                                     G_hi=g2t[0, :, t * n:].data_ptr(), G_lo=g2t[1, :, t * n:].data_ptr())
    check(L.eegclip_infonce_fused_grad(ga_, T_, n, N, Dm, planes, n, sc.data_ptr(), acc.data_ptr() + 4, st), "infonce_fused_grad")
    check(L.eegclip_infonce_fused_grad(gb_, T_, N, n, Dm, planes, n, sc.data_ptr(), acc.data_ptr() + 4, st), "infonce_fused_grad (transposed)")
    da = add_slabs(query_grad_slabs(g1, tall, n, T_ * N, Dm)[0])
    S2 = int(L.eegclip_head_gemm_slices(N, Dm, T_ * n))
    gas = torch.empty(S2, N, Dm, dtype=torch.float32, device=dev)
    d = _abi.HeadGemmDesc(a_hi=g2t[0].data_ptr(), a_lo=g2t[1].data_ptr(), b_hi=tloc[0].data_ptr(), b_lo=tloc[1].data_ptr(), lda=T_ * n, ldb=Dm, M=N, N=Dm,
                          K=T_ * n, slices=S2, slab_stride=N * Dm, C=gas.data_ptr(), ldc=Dm, b_kmajor=1)
    check(L.eegclip_head_gemm(ctypes.byref(d), st), "head_gemm")
    da._eegclip_keep = (buf, qa, tall, tloc)
    return da, add_slabs(gas)


def sharded_blocks(local_loss, gather_with_grad, rank, W, a_, bs, a_all, b_alls, weights, sc, acc, need_a, need_b, need, planes, bf16_logits=False):
    """What ONE rank computes between the collectives of a data-parallel ClipLoss (models/loss.py:100-141 with world_size > 1): the loss / d scale
    contributions (added to `acc`) and
        da       (n, D)   gradient w.r.t. this rank's own query rows (the part that does not travel),
        ga       (N, D)   gradient w.r.t. the GATHERED query copies, summed over the targets (local_loss + gather_with_grad), else None
        dbs[t]   (n, D)   gradient w.r.t. this rank's rows of target t, gbs[t] (N, D) its gathered-copy part (to be reduce-scattered) or None.
    No collective is issued here: the caller all-gathers before and reduce-scatters after (tests drive it rank by rank on one GPU)."""
    n, Dm = a_.shape
    N = W * n
    PX3 = _abi.PREC_BF16X3
    sl = slice(rank * n, (rank + 1) * n)
    da, ga = None, None
    dbs, gbs = [None] * len(bs), [None] * len(bs)
    fused = fused_enabled(n, N, Dm) and all(b.shape == a_.shape for b in bs)
    if (fused and local_loss and gather_with_grad and need and need_a and not any(need_b) and len(bs) <= 8 and head_gemm_enabled(n, len(bs) * N, Dm)):
        da, ga = _sharded_blocks_on_planes(rank, W, a_, bs, a_all, b_alls, weights, sc, acc, planes)
        return da, ga, dbs, gbs
    if fused:
        a_all_p = split_planes(a_all, planes)
        ap = (a_all_p[0][sl], a_all_p[1][sl] if planes == 2 else None)        # this rank's rows of the gathered planes
    for t, (b_, w) in enumerate(zip(bs, weights)):
        b_all = b_alls[t]
        if fused:
            b_all_p = split_planes(b_all, planes)
            bp = (b_all_p[0][sl], b_all_p[1][sl] if planes == 2 else None)
            if not local_loss:
                # every rank scores the full N x N matrix (models/loss.py:117-121): both terms from one gradient matrix
                Gs = fused_infonce([(a_all_p, b_all_p, 0, 0.5 * w), (b_all_p, a_all_p, 0, 0.5 * w)], N, N, Dm, planes, N, sc, acc,
                                   [(0, 1)] if need else [])
                if not need:
                    continue
                G = Gs[0]
                mult = float(W) if gather_with_grad else 1.0
                if need_a:
                    part = _grad_rows(G[sl], b_all, None, PX3) * mult
                    da = part if da is None else da + part
                if need_b[t]:
                    dbs[t] = _grad_cols(G, a_all, None, PX3)[sl] * mult
            else:
                # row-sharded (models/loss.py:113-115,129-130): this rank's rows against everybody's, positives at column i + n*rank
                Gs = fused_infonce([(ap, b_all_p, rank * n, 0.5 * w), (bp, a_all_p, rank * n, 0.5 * w)], n, N, Dm, planes, n, sc, acc,
                                   [(0, None), (1, None)] if need else [])
                if not need:
                    continue
                G1, G2 = Gs
                if need_a:
                    da = _grad_rows(G1, b_all, da, PX3)
                if need_b[t]:
                    dbs[t] = _grad_rows(G2, a_all, None, PX3)
                if gather_with_grad:
                    if need_a:
                        ga = _grad_cols(G2, b_, ga, PX3)
                    if need_b[t]:
                        gbs[t] = _grad_cols(G1, a_, None, PX3)
            continue
        if not local_loss:
            # every rank scores the full N x N matrix (models/loss.py:117-121)
            _, _, X = infonce_block(a_all, b_all, sc, 0, W * n, w, True, True, need, acc, bf16_logits)
            mult = float(W) if gather_with_grad else 1.0     # all_gather backward sums W identical copies
            if need_a:
                part = _grad_rows(X[sl].contiguous(), b_all) * mult
                da = part if da is None else da + part
            if need_b[t]:
                dbs[t] = _grad_cols(X, a_all)[sl] * mult
        else:
            # row-sharded: n x N blocks, positives at column i + n*rank (models/loss.py:113-115,129-130)
            _, _, X1 = infonce_block(a_, b_all, sc, rank * n, n, w, True, False, True, acc)
            _, _, X2 = infonce_block(b_, a_all, sc, rank * n, n, w, True, False, True, acc)
            if need_a:
                da = _grad_rows(X1, b_all, da)
            if need_b[t]:
                dbs[t] = _grad_rows(X2, a_all)
            if gather_with_grad:
                if need_a:
                    ga = _grad_cols(X2, b_, ga)                   # (N, D): d loss_r / d a_all, summed over the targets
                if need_b[t]:
                    gbs[t] = _grad_cols(X1, a_)
    return da, ga, dbs, gbs


_ACC_POOL = {}


def _zero_pair(dev):
    """a zeroed (loss, dscale) accumulator pair: slices of a pool that is filled 128 pairs at a time (one fill launch per 128 loss calls instead of
    one per call; a slice is handed out once, so a loss value that is still referenced is never overwritten)"""
    key = str(dev)
    pool, used = _ACC_POOL.get(key, (None, 0))
    if pool is None or used >= pool.shape[0]:
        pool, used = torch.zeros(128, 2, dtype=torch.float32, device=dev), 0
    _ACC_POOL[key] = (pool, used + 1)
    return pool[used]


class _ClipLossFn(torch.autograd.Function):
    """loss = sum_t w_t * ClipLoss(a, b_t, scale) for one or more target matrices b_t that share the query features `a`
    (the training loop mixes an image and a text target, ATMS_retrieval.py:224-229): one (loss, dscale) accumulator, one gradient
    w.r.t. `a` (the second target's dA GEMM accumulates onto the first), a_all gathered once, and -- data parallel -- ONE
    reduce-scatter for the gradients that reached the gathered copies of `a`."""

    @staticmethod
    def forward(ctx, a, scale_t, mod, weights, *targets):
        dev = a.device
        sc = _scale_ptr(scale_t, dev)
        need_a = a.requires_grad
        need_b = [b.requires_grad for b in targets]
        need_s = torch.is_tensor(scale_t) and scale_t.requires_grad
        need = need_a or any(need_b) or need_s
        W, rank = mod.world_size, mod.rank
        a_ = a.detach().contiguous()
        bs = [b.detach().contiguous() for b in targets]
        n = a_.shape[0]
        acc = _zero_pair(dev)
        da = None
        dbs = [None] * len(bs)
        planes = 2 if mod.logits_dtype == "f32" else 1
        PX3 = _abi.PREC_BF16X3                              # the dQ = G K / dK = G^T Q GEMMs behind the fused kernels: split-bf16 products too
        Dm = a_.shape[1]
        # (batches that are not whole 64-tiles: only the small form -- K-parallel logits GEMM + row-block kernels -- takes them, and only to train the queries)
        # (under EEGCLIP_GEMM_PRECISION=f32 such batches keep the exact-fp32 GEMM + log-sum-exp route: the reference fixtures at B = 16 hold that arithmetic to 2e-4)
        from .plan import default_gemm_precision
        can_small = (need_a and need and not any(need_b) and default_gemm_precision() == PX3 and head_gemm_enabled(n, len(bs) * n, Dm)
                     and infonce_small_enabled(n, len(bs), planes))
        if W == 1 and (fused_enabled(n, n, Dm) or can_small) and all(b.shape == a_.shape for b in bs):
            # blocks (A, B_t) and (B_t, A) of every target in ONE launch; one gradient matrix per target with both normalisers
            # query gradient of T >= 2 targets as ONE contraction over the stacked targets: dA = [G_1 | .. | G_T] [B_1; ..; B_T] -- the gradient matrices
            # side by side in one (n, T n) buffer, the targets stacked by the launch that splits them (T GEMM launches of K = n -> one of K = T n)
            T_ = len(bs)
            stacked = need_a and T_ >= 2
            # (round 6) ... on the K-parallel plane GEMM when nothing else needs the fp32 gradient matrices: G leaves the gradient pass as planes, the
            # targets are split transposed, dA = the GEMM's slabs added in slice order (the step plan hands the slabs to the encoder's backward as they are)
            on_planes = need_a and need and not any(need_b) and head_gemm_enabled(n, T_ * n, Dm)
            stack = torch.empty(T_ * n, Dm, dtype=torch.float32, device=dev) if stacked and not on_planes else None
            small = on_planes and infonce_small_enabled(n, T_, planes)
            if on_planes:
                ap, bps, tp, aq = stacked_target_planes(a_, bs, planes)
            else:
                ap, *bps = split_planes_many([a_] + bs, planes, stack)
            blocks, want = [], []
            for t, w in enumerate(weights):
                blocks += [(ap, bps[t], 0, 0.5 * w), (bps[t], ap, 0, 0.5 * w)]
                want.append((2 * t, 2 * t + 1))
            if on_planes:
                Gp = torch.empty(2, n, T_ * n, dtype=torch.bfloat16, device=dev)
                if small:
                    infonce_small(aq, tp, n, T_, Dm, weights, sc, acc, Gp)
                else:
                    fused_infonce(blocks, n, n, Dm, planes, n, sc, acc, want, None, [(Gp[0, :, t * n:(t + 1) * n], Gp[1, :, t * n:(t + 1) * n]) for t in range(T_)])
                da = add_slabs(query_grad_slabs(Gp, tp, n, T_ * n, Dm)[0])
                stacked, Gs = False, None
                need_a = False                                    # (da is complete)
            Gcat = torch.empty(n, T_ * n, dtype=torch.float32, device=dev) if stacked and need else None
            if not on_planes:
                Gs = fused_infonce(blocks, n, n, Dm, planes, n, sc, acc, want if need else [],
                                   [Gcat[:, t * n:(t + 1) * n] for t in range(T_)] if Gcat is not None else None)
            if stacked and need:
                da = _grad_rows(Gcat, stack, None, PX3)
            for t, b_ in enumerate(bs):
                if need_a and not stacked:
                    da = _grad_rows(Gs[t], b_, da, PX3)
                if need_b[t]:
                    dbs[t] = _grad_cols(Gs[t], a_, None, PX3)
        elif W == 1:
            for t, (b_, w) in enumerate(zip(bs, weights)):
                _, _, X = infonce_block(a_, b_, sc, 0, n, w, True, True, need, acc, mod.logits_dtype == "bf16")
                if need_a:
                    da = _grad_rows(X, b_, da)
                if need_b[t]:
                    dbs[t] = _grad_cols(X, a_)
        else:
            import torch.distributed as dist
            a_all = torch.empty(W * n, a_.shape[1], dtype=torch.float32, device=dev)
            dist.all_gather_into_tensor(a_all, a_)
            b_alls = mod._gathered_targets(bs)                     # ONE all-gather for every target (usually started at step start)
            da, ga, dbs, gbs = sharded_blocks(mod.local_loss, mod.gather_with_grad, rank, W, a_, bs, a_all, b_alls, weights, sc, acc, need_a, need_b,
                                              need, planes, mod.logits_dtype == "bf16")
            # gradients that reached the GATHERED copies flow back through all_gather = reduce-scatter(sum) (models/loss.py:52-58)
            for t_, gb in enumerate(gbs):
                if gb is not None:
                    part = torch.empty_like(bs[t_])
                    dist.reduce_scatter_tensor(part, gb)
                    dbs[t_] = dbs[t_] + part
            if ga is not None:
                part = torch.empty_like(a_)
                dist.reduce_scatter_tensor(part, ga)
                da = da + part
        ctx.grads = (da, acc[1].reshape(()) if need_s else None, dbs)
        ctx.unit_grad = bool(getattr(mod, "_unit_upstream_grad", False))
        return acc[0].reshape(())

    @staticmethod
    def backward(ctx, go):
        da, ds, dbs = ctx.grads
        if ctx.unit_grad:
            # the caller guarantees that this loss is the root of the backward pass (upstream gradient == 1: the batch loop of retrieval.py calls
            # loss.backward() on exactly this scalar): the gradients computed in forward are returned as they are -- two elementwise launches
            # (dA * 1, dscale * 1) less on the critical path between the loss and the encoder's backward
            return (da, ds, None, None) + tuple(dbs)
        return (da * go if da is not None else None, ds * go if ds is not None else None, None, None) + \
            tuple(db * go if db is not None else None for db in dbs)


class ClipLoss(nn.Module):
    def __init__(self, local_loss=False, gather_with_grad=False, cache_labels=False, rank=0, world_size=1, use_horovod=False,
                 logits_dtype="f32"):
        """logits_dtype (extension, default = the reference's fp32 semantics): "bf16" computes the N x N logits of a full-matrix block on
        the bf16 matrix cores (features rounded to bf16, fp32 accumulate / logits / gradients) when N % 128 == 0 and D % 64 == 0 -- the
        large-global-batch configuration; the logit error is ~2^-9 of |a||b| per term (3e-2 at |logit| ~ 16), outside the 1e-3 parity
        budget, hence opt-in."""
        super().__init__()
        if logits_dtype not in ("f32", "bf16"):
            raise ValueError("logits_dtype must be 'f32' or 'bf16'")
        self.logits_dtype = logits_dtype
        if use_horovod:
            raise NotImplementedError("horovod is not part of the MI355X build; use torch.distributed (RCCL)")
        self.local_loss = local_loss
        self.gather_with_grad = gather_with_grad
        self.cache_labels = cache_labels      # labels are implicit (diagonal + rank offset) in the kernels; kept for API parity
        self.rank = rank
        self.world_size = world_size
        self.use_horovod = use_horovod

    # ---- data parallel: the targets are INPUTS of the step (frozen CLIP features), so their all-gather does not have to wait for the encoder ----
    @staticmethod
    def _target_key(ts):
        return tuple((t.data_ptr(), tuple(t.shape), t._version) for t in ts)

    def gather_targets(self, *targets):
        """Start ONE asynchronous all-gather of all the step's target matrices ([img | txt] stacked, (T, n, D) per rank -> (W, T, n, D)) -- call it
        before the encoder forward; the next forward / forward_mixed on the SAME tensors picks the result up and only then waits for it.  No-op
        for a single process.  (The reference gathers inside the loss, models/loss.py:20-75: same values, issued earlier.)"""
        if self.world_size <= 1:
            return None
        import torch.distributed as dist
        ts = [t.detach().contiguous() for t in targets]
        if any(t.shape != ts[0].shape or t.dtype != torch.float32 for t in ts):
            return None                                           # (ragged targets: gathered one by one inside the loss)
        send = ts[0].unsqueeze(0) if len(ts) == 1 else torch.stack(ts)
        out = torch.empty((self.world_size * send.shape[0],) + tuple(send.shape[1:]), dtype=torch.float32, device=send.device)
        work = dist.all_gather_into_tensor(out, send, async_op=True)
        self._pending_targets = (self._target_key(ts), work, out, send)
        return work

    def _gathered_targets(self, bs):
        """[(W n, D) gathered copy of every target]: the prefetched gather if it was started for exactly these tensors, else one gather now."""
        import torch.distributed as dist
        pend, self._pending_targets = getattr(self, "_pending_targets", None), None
        if pend is not None and pend[0] == self._target_key(bs):
            pend[1].wait()
            out = pend[2]
        elif all(b.shape == bs[0].shape for b in bs):
            send = bs[0].unsqueeze(0) if len(bs) == 1 else torch.stack(bs)
            out = torch.empty((self.world_size * send.shape[0],) + tuple(send.shape[1:]), dtype=torch.float32, device=send.device)
            dist.all_gather_into_tensor(out, send)
        else:
            res = []
            for b in bs:
                b_all = torch.empty(self.world_size * b.shape[0], b.shape[1], dtype=torch.float32, device=b.device)
                dist.all_gather_into_tensor(b_all, b)
                res.append(b_all)
            return res
        W, n = self.world_size, bs[0].shape[0]
        if len(bs) == 1:
            return [out.view(W * n, -1)]
        out = out.view(W, len(bs), n, -1)                       # (rank, target, sample, feature)
        return [out[:, t].reshape(W * n, -1) for t in range(len(bs))]        # (rank, sample) rows of target t, contiguous

    def forward(self, image_features, text_features, logit_scale):
        require_cuda(image_features, "image_features")
        require_cuda(text_features, "text_features")
        if image_features.dtype != torch.float32 or text_features.dtype != torch.float32:
            raise TypeError("ClipLoss expects float32 features (the reference casts with .float())")
        return _ClipLossFn.apply(image_features, logit_scale, self, (1.0,), text_features)

    def forward_mixed(self, features, targets, logit_scale):
        """sum_t w_t * self(features, target_t, logit_scale) in one pass; targets = [(tensor, weight), ...].  Equal (up to fp32
        summation order) to calling forward per target and mixing the scalars, which is what the reference loop does."""
        require_cuda(features, "features")
        for b, _ in targets:
            require_cuda(b, "target")
            if b.dtype != torch.float32:
                raise TypeError("ClipLoss expects float32 features (the reference casts with .float())")
        if features.dtype != torch.float32:
            raise TypeError("ClipLoss expects float32 features (the reference casts with .float())")
        return _ClipLossFn.apply(features, logit_scale, self, tuple(float(w) for _, w in targets), *[b for b, _ in targets])


class _MseFn(torch.autograd.Function):
    """weight * mean((pred - target)^2) and its gradient w.r.t. pred in one kernel pass (nn.MSELoss of
    Generation/ATMS_reconstruction.py:201,227; also the diffusion prior's objective)."""

    @staticmethod
    def forward(ctx, pred, target, weight):
        require_cuda(pred, "pred")
        p, t = pred.detach().contiguous(), target.detach().contiguous()
        acc = torch.zeros(1, dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p) if pred.requires_grad else None
        check(lib().eegclip_mse_loss_grad(p.data_ptr(), t.data_ptr(), p.numel(), acc.data_ptr(), grad.data_ptr() if grad is not None else None,
                                          _stream()), "mse_loss_grad")
        ctx.grad, ctx.weight = grad, float(weight)
        return acc.reshape(()) * float(weight)

    @staticmethod
    def backward(ctx, go):
        return (ctx.grad * (go * ctx.weight) if ctx.grad is not None else None), None, None


def mse_loss(pred, target, weight=1.0):
    if pred.dtype != torch.float32 or target.dtype != torch.float32 or pred.shape != target.shape:
        raise TypeError("mse_loss expects two float32 tensors of the same shape")
    return _MseFn.apply(pred, target, weight)
