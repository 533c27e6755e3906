"""git_caption.GITCaptioner at GIT-large's shapes (6 layers, 768 wide, vocabulary 30522; P = 257 image tokens, max_length 20, fp16), B = 1 and B = 8.
Writes one JSON object (default profiles/git_caption_bench.json):

* prefill_ms: the prefill over the image tokens and bos (cache filled) plus the LM head of the last row, median of --reps synchronised runs.
* per_token_ms: one decoding step (greedy choice with its host read, then the step's 58 launches), median over the 19 steps of a caption, repeated --reps times.
* lower_bound_ms: the bytes of every weight a step reads once (six layers + the LM head) over the 8.0 TB/s HBM rate bench.py uses; fraction_reached =
  lower_bound / measured.  (At these sizes the weights, 132 MB, fit the 256 MiB Infinity Cache: the bound is the HBM figure all the same.)
* ab_gemm16: the same decoding step with its GEMMs on csrc/gemm16.hip (M padded inside its 128-row tile; k | v copied into the cache row by a separate
  launch; the LM head over a weight padded to 30592 rows, built here for the comparison only) against csrc/caption.hip's skinny GEMM, alternated in ONE
  process: median, min, max of each and skinny / gemm16.

* gemm_kernels: the step's six GEMM shapes (q; k | v; dense; intermediate; output.dense; LM head) one launch at a time, each kernel's own begin .. end
  timestamps (eegclip_time_next_launch), skinny and gemm16 alternated, median of 15: kernel time without launch gaps, bytes of W over it, and the sum per
  token (five shapes x six layers + the LM head).

Each batch size is measured in a fresh worker process under its own time limit; a worker that fails ends the run.

    python tools/bench_git_caption.py [--reps 7] [--out profiles/git_caption_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8.0e12
P, MAX_LENGTH = 257, 20


def _sync_ms(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread": round((max(v) - min(v)) / statistics.median(v), 4)}


def worker(B, reps):
    import torch
    from eeg_image_decode_amd.git_caption import GELU, GITCaptioner
    from eeg_image_decode_amd.ops16 import act16, decode_attention, gather_rows16, layernorm16, linear16, linear16_skinny
    if not torch.cuda.is_available():
        raise SystemExit("bench_git_caption.py measures on the GPU; none found")
    m = GITCaptioner(device="cuda", dtype=torch.float16)
    cfg = m.config
    C, V, L = cfg.hidden_size, cfg.vocab_size, cfg.num_hidden_layers
    vis = torch.randn(B, P, cfg.vision_hidden_size, device="cuda", dtype=torch.float16, generator=torch.Generator(device="cuda").manual_seed(B))
    ids = torch.full((B, 1), cfg.bos_token_id)
    cache = torch.empty(L, B, P + MAX_LENGTH, 2 * C, dtype=torch.float16, device="cuda")

    def prefill():
        x = m._prefill(ids, vis, cache)
        return linear16_skinny(x[:, P], m.output.weight, m.output.bias, out_f32=True)

    # ---- the step with its GEMMs on gemm16 (the comparison only) ----
    pad = (V + 127) // 128 * 128
    w_pad = torch.zeros(pad, C, dtype=torch.float16, device="cuda")
    w_pad[:V] = m.output.weight
    b_pad = torch.zeros(pad, dtype=torch.float16, device="cuda")
    b_pad[:V] = m.output.bias

    def step_gemm16(tok, t):
        g, ln = m.git, lambda x, mod: layernorm16(x, mod.weight, mod.bias, mod.eps)
        emb = g.embeddings
        x = ln(gather_rows16(emb.word_embeddings.weight, tok.cuda(), B, emb.position_embeddings.weight[t:t + 1], 1), emb.LayerNorm)
        for i, layer in enumerate(g.encoder.layer):
            att = layer.attention
            w, b = m._packed(i, att.self)
            qkv = linear16(x, w, b)
            cache[i, :, P + t] = qkv[:, C:]
            a = decode_attention(qkv[:, :C], cache[i], P + t + 1, cfg.num_attention_heads)
            x = ln(linear16(a, att.output.dense.weight, att.output.dense.bias, x), att.output.LayerNorm)
            f = act16(linear16(x, layer.intermediate.dense.weight, layer.intermediate.dense.bias), GELU)
            x = ln(linear16(f, layer.output.dense.weight, layer.output.dense.bias, x), layer.output.LayerNorm)
        return linear16(x, w_pad, b_pad)[:, :V].float()

    def caption(step):
        """the 19 steps of a caption (no early stop: the timing is of the steps); per-step ms"""
        logits, ms = prefill(), []
        for t in range(1, MAX_LENGTH):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tok = m._greedy(logits)                                    # the host read of the step
            logits = step(tok, t)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, tok

    skinny = lambda tok, t: m._step(tok, t, P, cache)                   # noqa: E731
    with torch.no_grad():
        for _ in range(2):                                             # warm-up: code objects, the allocator's pool
            caption(skinny)
            caption(step_gemm16)
        pre = [_sync_ms(prefill) for _ in range(reps)]
        ms_s, ms_g = [], []
        for _ in range(reps):                                          # alternated
            a, tok_s = caption(skinny)
            b, tok_g = caption(step_gemm16)
            ms_s.append(statistics.median(a))
            ms_g.append(statistics.median(b))
    kernels = gemm_kernels(m, B, w_pad, b_pad)
    wbytes = 2 * (L * (4 * C * C + 2 * C * cfg.intermediate_size + 9 * C + cfg.intermediate_size) + V * C + V)
    bound = wbytes / HBM_BYTES_PER_S * 1e3
    s, g = _stats(ms_s), _stats(ms_g)
    print(json.dumps({"B": B, "P": P, "max_length": MAX_LENGTH, "dtype": "float16", "repetitions": reps, "prefill": _stats(pre), "per_token": s,
                      "launches_per_token": 9 * L + 4, "weight_bytes_per_token": wbytes, "lower_bound_ms": round(bound, 4),
                      "fraction_reached": round(bound / s["median_ms"], 4),
                      "gemm_kernels": kernels,
                      "ab_gemm16": {"gemm16": g, "skinny": s, "skinny_over_gemm16": round(s["median_ms"] / g["median_ms"], 4),
                                    "same_last_token": bool(torch.equal(tok_s, tok_g))}}), flush=True)


def gemm_kernels(m, B, w_pad, b_pad):
    import torch
    from eeg_image_decode_amd._lib import lib
    from eeg_image_decode_amd.ops16 import linear16, linear16_skinny
    L_, cfg = lib(), m.config
    C, I, V, nl = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    e0, e1 = L_.eegclip_timing_event_create(), L_.eegclip_timing_event_create()

    def stamped(f):
        torch.cuda.synchronize()
        assert L_.eegclip_time_next_launch(e0, e1) == 0
        f()
        torch.cuda.synchronize()
        return float(L_.eegclip_timing_elapsed_ms(e0, e1))

    layer, wq, bq = m.git.encoder.layer[0], *m._packed(0, m.git.encoder.layer[0].attention.self)
    x, xi = torch.randn(B, C, device="cuda").half(), torch.randn(B, I, device="cuda").half()
    shapes = [("q", x, wq[:C], bq[:C], nl), ("k|v", x, wq[C:], bq[C:], nl), ("attention.output.dense", x, layer.attention.output.dense.weight,
              layer.attention.output.dense.bias, nl), ("intermediate.dense", x, layer.intermediate.dense.weight, layer.intermediate.dense.bias, nl),
              ("output.dense", xi, layer.output.dense.weight, layer.output.dense.bias, nl), ("lm_head", x, m.output.weight, m.output.bias, 1)]
    rows, tot = [], {"skinny": 0.0, "gemm16": 0.0}
    for name, a, w, b, per_token in shapes:
        w16, b16 = (w_pad, b_pad) if name == "lm_head" else (w, b)
        run = {"skinny": lambda: linear16_skinny(a, w, b, out_f32=name == "lm_head"), "gemm16": lambda: linear16(a, w16, b16)}
        for f in run.values():
            f(), f()
        ms = {k: [] for k in run}
        for _ in range(15):
            for k, f in run.items():                                    # alternated
                ms[k].append(stamped(f))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in tot:
            tot[k] += per_token * med[k]
        rows.append({"gemm": name, "M": B, "N": w.shape[0], "K": w.shape[1], "per_token": per_token, "skinny_us": round(med["skinny"] * 1e3, 2),
                     "gemm16_us": round(med["gemm16"] * 1e3, 2), "skinny_min_us": round(min(ms["skinny"]) * 1e3, 2), "gemm16_min_us": round(min(ms["gemm16"]) * 1e3, 2),
                     "skinny_W_TBps": round(2.0 * w.shape[0] * w.shape[1] / med["skinny"] / 1e9, 3)})
    L_.eegclip_timing_event_destroy(e0), L_.eegclip_timing_event_destroy(e1)
    return {"shapes": rows, "sum_per_token_us": {k: round(v * 1e3, 1) for k, v in tot.items()}, "skinny_over_gemm16": round(tot["skinny"] / tot["gemm16"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "git_caption_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.worker:
        return worker(args.worker, args.reps)
    rows = []
    for B in (1, 8):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(B), "--reps", str(args.reps)], cwd=ROOT, stdout=subprocess.PIPE, text=True,
                           timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit(f"the worker for B = {B} ended with status {r.returncode}; nothing further is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "model": "GITCaptioner() defaults (GIT-large's text decoder), seeded weights", "cases": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
