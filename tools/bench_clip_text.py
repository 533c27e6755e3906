"""SDXL's two CLIP text encoders (eeg_image_decode_amd/clip_text.py) on the GPU: encode time of each encoder, fp16, for B = 1 and B = 16 prompts of 77 ids
(median of N timed forwards after a warm-up, each forward ending in a device synchronise -- the ids go up and the pooling index is built on the host, as in
a real call), kernel launches per forward (from the layer structure: 8 per layer + embedding, final LayerNorm, pooling, projection), and beside it the
same weights through transformers' CLIPTextModel / CLIPTextModelWithProjection on the same GPU when transformers imports.  Prints one JSON object.

    python tools/bench_clip_text.py [--out profiles/clip_text_bench.json] [--repeats 30]
    python tools/bench_clip_text.py --profile-pass        # a few forwards only: the program to put under rocprofv3 --kernel-trace --stats
    python tools/bench_clip_text.py --kernel-stats DIR     # fold rocprofv3's *_kernel_stats.csv under DIR into the per-family split (no GPU needed)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = (("gemm", ("gemm16",)), ("attention", ("self_attn_kernel",)), ("layernorm", ("layernorm16",)), ("activation", ("act16",)),
            ("gather", ("gather_rows16",)))


SETUP = "setup (torch: weight init, fp16 cast, q|k|v packing, id upload)"


def family_of(kernel_name, families=FAMILIES, setup=SETUP):
    for fam, keys in families:
        if any(k in kernel_name for k in keys):
            return fam
    return setup if ("at::native" in kernel_name or "__amd_rocclr" in kernel_name) else "other"


def kernel_split(directory, families=FAMILIES, setup=SETUP):
    """rocprofv3 --kernel-trace --stats output -> {family: {"calls", "ms", "share_of_forward"}} over the kernels of the traced run.  families: (name, kernel
    name substrings) pairs; setup: the label of torch's own kernels (building the model), kept out of the shares"""
    fam = {}
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                e = fam.setdefault(family_of(row["Name"], families, setup), {"calls": 0, "ms": 0.0})
                e["calls"] += int(row["Calls"])
                e["ms"] += float(row["TotalDurationNs"]) / 1e6
    total = sum(e["ms"] for k, e in fam.items() if k != setup)          # shares over the forward's own kernels: building the model is not encoding
    return {k: dict({"calls": e["calls"], "ms": round(e["ms"], 3)}, **({} if k == setup else {"share_of_forward": round(e["ms"] / total, 3)}))
            for k, e in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])}


def ids_batch(B):
    import torch
    g = torch.Generator().manual_seed(B)
    rows = []
    for b in range(B):
        n = [9, 40, 75, 20][b % 4]
        body = torch.randint(1, 49406, (n,), generator=g).tolist()
        rows.append([49406] + body + [49407] * (76 - n))
    return torch.tensor(rows)


def timed(f, repeats, warmup=5):
    import torch
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "repeats": repeats}


def hf_twin(enc):
    """the same weights in transformers' model on the GPU, or None when transformers does not import"""
    try:
        import transformers
    except ImportError:
        return None
    c = enc.config
    cfg = transformers.CLIPTextConfig(vocab_size=c.vocab_size, hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                                      num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads, hidden_act=c.hidden_act,
                                      projection_dim=c.projection_dim or c.hidden_size, max_position_embeddings=c.max_position_embeddings,
                                      layer_norm_eps=c.layer_norm_eps, eos_token_id=2, bos_token_id=0, pad_token_id=1)
    cls = transformers.CLIPTextModelWithProjection if c.projection_dim is not None else transformers.CLIPTextModel
    m = cls(cfg).to(enc.dtype).eval()
    have = set(m.state_dict())
    sd = {(k if k in have else k[len("text_model."):]): v for k, v in enc.state_dict().items()}        # (CLIPTextModel's keys may lack the prefix)
    m.load_state_dict(sd)
    return m.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--no-transformers", action="store_true")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps({"kernel_families": kernel_split(a.kernel_stats)}))
        return
    import torch
    from eeg_image_decode_amd import clip_text
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_text.py measures on the GPU; none found")
    out = {"dtype": "float16", "tokens": 77, "timing": "host clock around forward + device synchronise; median", "encoders": {}}
    with torch.no_grad():
        for name, make in (("text_encoder", clip_text.sdxl_text_encoder), ("text_encoder_2", clip_text.sdxl_text_encoder_2)):
            enc = make(dtype=torch.float16, device="cuda")
            if a.profile_pass:
                for B in (1, 16):
                    ids = ids_batch(B)
                    for _ in range(3):
                        enc(ids, output_hidden_states=True)
                torch.cuda.synchronize()
                del enc
                continue
            res = {"parameters": sum(p.numel() for p in enc.parameters()), "layers": enc.config.num_hidden_layers,
                   "launches_per_forward": 8 * enc.config.num_hidden_layers + 3 + (enc.config.projection_dim is not None)}
            twin = None if a.no_transformers else hf_twin(enc)
            for B in (1, 16):
                ids = ids_batch(B)
                r = timed(lambda: enc(ids, output_hidden_states=True), a.repeats)
                c = enc.config
                M = B * 77
                flop = c.num_hidden_layers * (2.0 * M * c.hidden_size * (4 * c.hidden_size + 2 * c.intermediate_size) + 4.0 * B * 77 * 77 * c.hidden_size / 2)
                r["TFLOPs_end_to_end"] = round(flop / r["median_ms"] / 1e9, 2)                    # whole-forward rate (causal attention counted at half)
                if twin is not None:                                                              # same ids, same weights, transformers' own forward
                    dev_ids = ids.cuda()
                    t = timed(lambda: twin(input_ids=dev_ids, output_hidden_states=True), a.repeats)
                    r["transformers_median_ms"] = t["median_ms"]
                    got = enc(ids, output_hidden_states=True)
                    want = twin(input_ids=dev_ids, output_hidden_states=True)
                    r["rel_l2_hidden_states_m2_vs_transformers_fp16"] = float(f"{float((got.hidden_states[-2].float() - want.hidden_states[-2].float()).norm() / want.hidden_states[-2].float().norm()):.3e}")
                res[f"B{B}"] = r
            if twin is None:
                res["transformers"] = "not measured (transformers does not import here)" if not a.no_transformers else "not measured (--no-transformers)"
            out["encoders"][name] = res
            del enc, twin
            torch.cuda.empty_cache()
    if a.profile_pass:
        print(json.dumps({"profile_pass": "3 forwards of each encoder at B = 1 and B = 16"}))
        return
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
