"""CLIP's vision towers (eeg_image_decode_amd/clip_vision.py) and the attention kernel at head dim 80 (csrc/self_attn.hip's template) on the GPU.  Prints one JSON object.

  attention  csrc/self_attn.hip at head dim 80 (eegclip_attn80_fwd; `attn80` in the rows) at (B, T, heads) = (1 | 16 | 256, 257, 16), fp16 and bf16, on a fused (B, T, 3C) buffer: microseconds and the fraction of the
             2.5 PF/s dense 16-bit peak in USEFUL FLOPs (4 B heads T T 80: the zero half of the third k-step is not counted); beside each the 64-wide
             instantiation at the same B, T, heads (4 B heads T T 64) and torch's scaled_dot_product_attention at head dim 80 on the same tensors.
             `cost_per_useful_flop_vs_64` = (attn80 us / its FLOPs) / (64-wide us / its FLOPs): 96 / 80 = 1.2 is what the padded third k-step alone costs.
  towers     ip_adapter_image_encoder() and git_vision_tower(), fp16, ms per image at B = 1, 16, 64; beside it transformers' own model with the same
             weights in fp16 on the same GPU; the C-ABI calls of one forward, counted (each is one kernel launch: 3 to hidden_states[0], 8 per layer,
             post_layernorm, projection).

Every figure is the median of `--windows` event-bracketed windows of many iterations after a warm-up of every shape; min / max of the windows are the
spread.  The three attention kernels alternate inside a round of windows, so that a drift of the shared machine hits them alike.

    python tools/bench_clip_vision.py [--out profiles/clip_vision_bench.json] [--windows 7]
    python tools/bench_clip_vision.py --profile-pass       # a few forwards only: the program to put under rocprofv3 --kernel-trace --stats
    python tools/bench_clip_vision.py --kernel-stats DIR [--out FILE]   # fold rocprofv3's *_kernel_stats.csv under DIR into the per-family split (no GPU needed)

--out FILE updates FILE: the keys this run computes are replaced, every other key of an existing FILE stays (`kernel_families` from a --kernel-stats run,
`model_errors` = the figures tests/test_clip_vision_gpu.py prints, `query_block_ab` = the 64 | 128 queries per workgroup comparison taken with a second
build at head dim 80, two query tiles per wave, that is not in the tree); each of those sections says where it came from.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_clip_text import kernel_split  # noqa: E402  (the rocprofv3 kernel_stats reader)

PEAK = 2.5e15
T, HEADS = 257, 16
FAMILIES = (("gemm", ("gemm16",)), ("attention", ("self_attn_kernel",)), ("layernorm", ("layernorm16", "embed_ln16")),
            ("activation", ("act16",)), ("patch rows", ("patch_rows16",)))
# attention: both towers run instantiations of one template (head dim 80 and 64), whose names begin alike; the traced pass runs nothing else that matches
SETUP = "setup (torch: weight init, fp16 cast, q|k|v and patch-weight packing, random pixels)"


def update_json(path, new):
    """write `new` into the JSON object at `path`, keeping the keys of an existing file that `new` does not have"""
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    old.update(new)
    with open(path, "w") as f:
        f.write(json.dumps(old, indent=1) + "\n")


def abi_calls(forward):
    """the C-ABI calls one call of `forward` makes, by name, counted through a proxy in front of the loaded library (ops16's wrappers fetch it per call)"""
    from eeg_image_decode_amd import ops16
    calls = {}

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)

            def counted(*a):
                calls[name] = calls.get(name, 0) + 1
                return fn(*a)
            return counted

    real = ops16.lib
    ops16.lib = lambda: Counting(real())
    try:
        forward()
    finally:
        ops16.lib = real
    return calls


def window_us(f, n):
    """one event-bracketed window of n calls -> microseconds per call"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def spread(us):
    return {"us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "windows": len(us)}


def attention_rows(windows):
    import torch
    import torch.nn.functional as F
    from eeg_image_decode_amd.ops16 import self_attention
    rows = []
    for dt in (torch.float16, torch.bfloat16):
        for B in (1, 16, 256):
            g = torch.Generator(device="cuda").manual_seed(B)
            fns, flops = {}, {}
            keep = []
            for d in (80, 64):
                C = HEADS * d
                qkv = torch.randn(B, T, 3 * C, device="cuda", dtype=dt, generator=g)
                q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
                o = torch.empty(B, T, C, device="cuda", dtype=dt)
                keep.append((qkv, o))
                fns[f"d{d}"] = (lambda q=q, k=k, v=v, o=o, d=d: self_attention(q, k, v, HEADS, out=o, head_dim=d))
                flops[f"d{d}"] = 4.0 * B * HEADS * T * T * d
                if d == 80:
                    qh, kh, vh = (t.reshape(B, T, HEADS, d).transpose(1, 2) for t in (q, k, v))
                    fns["sdpa80"] = (lambda qh=qh, kh=kh, vh=vh: F.scaled_dot_product_attention(qh, kh, vh))
            n = max(20, min(2000, int(4e11 / flops["d80"])))                 # windows of at least a few milliseconds
            for f in fns.values():                                            # warm-up of every shape
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            us = {k: [] for k in fns}
            for _ in range(windows):
                for k, f in fns.items():                                      # alternating
                    us[k].append(window_us(f, n))
            a80, a64, sd = spread(us["d80"]), spread(us["d64"]), spread(us["sdpa80"])
            cost = (a80["us"] / flops["d80"]) / (a64["us"] / flops["d64"])
            rel_spread = max((s["max_us"] - s["min_us"]) / s["us"] for s in (a80, a64))
            rows.append({"dtype": str(dt).split(".")[-1], "B": B, "T": T, "heads": HEADS, "iterations_per_window": n,
                         "attn80": dict(a80, useful_TFLOPs=round(flops["d80"] / a80["us"] / 1e6, 1), fraction_of_peak=round(flops["d80"] / a80["us"] / 1e-6 / PEAK, 4)),
                         "self_attn_64": dict(a64, TFLOPs=round(flops["d64"] / a64["us"] / 1e6, 1), fraction_of_peak=round(flops["d64"] / a64["us"] / 1e-6 / PEAK, 4)),
                         "torch_sdpa_80": dict(sd, useful_TFLOPs=round(flops["d80"] / sd["us"] / 1e6, 1)),
                         "cost_per_useful_flop_vs_64": round(cost, 3), "relative_spread_of_windows": round(rel_spread, 3)})
            del keep, fns
            torch.cuda.empty_cache()
    return rows


def hf_twin(enc):
    """the same weights in transformers' model on the GPU, or None when transformers does not import"""
    try:
        import transformers
    except ImportError:
        return None
    c = enc.config
    kw = dict(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
              hidden_act=c.hidden_act, image_size=c.image_size, patch_size=c.patch_size, layer_norm_eps=c.layer_norm_eps)
    if c.post_layernorm_all:
        m = transformers.GitVisionModel(transformers.GitVisionConfig(**kw))
    else:
        m = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(projection_dim=c.projection_dim, **kw))
    m = m.to(enc.dtype).eval()
    m.load_state_dict(enc.state_dict())
    return m.cuda()


def tower_rows(windows, with_transformers):
    import torch
    from eeg_image_decode_amd import clip_vision
    res = {}
    for name in ("ip_adapter_image_encoder", "git_vision_tower"):
        enc = getattr(clip_vision, name)(dtype=torch.float16, device="cuda")
        c = enc.config
        px1 = torch.zeros(1, 3, c.image_size, c.image_size, device="cuda", dtype=torch.float16)
        enc(px1)                                                              # (the weight packing happens here, outside the count)
        calls = abi_calls(lambda: enc(px1))
        r = {"parameters": sum(p.numel() for p in enc.parameters()), "layers": c.num_hidden_layers, "head_dim": c.hidden_size // c.num_attention_heads,
             "abi_calls_per_forward": sum(calls.values()), "abi_calls_by_entry_point": dict(sorted(calls.items()))}
        twin = hf_twin(enc) if with_transformers else None
        for B in (1, 16, 64):
            px = torch.randn(B, 3, c.image_size, c.image_size, device="cuda", dtype=torch.float16, generator=torch.Generator(device="cuda").manual_seed(B))
            fns = {"hip": lambda: enc(px)}
            if twin is not None:
                fns["transformers"] = lambda: twin(pixel_values=px)
            n = max(2, 32 // B)
            for f in fns.values():
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            us = {k: [] for k in fns}
            for _ in range(windows):
                for k, f in fns.items():
                    us[k].append(window_us(f, n))
            M = B * T
            flop = c.num_hidden_layers * (2.0 * M * c.hidden_size * (4 * c.hidden_size + 2 * c.intermediate_size) + 4.0 * B * T * T * c.hidden_size)
            row = {"iterations_per_window": n}
            for k, v in us.items():
                s = spread(v)
                row[k] = {"ms_per_image": round(s["us"] / 1e3 / B, 4), "min_ms_per_image": round(s["min_us"] / 1e3 / B, 4),
                          "max_ms_per_image": round(s["max_us"] / 1e3 / B, 4), "windows": s["windows"]}
            row["hip"]["TFLOPs_end_to_end"] = round(flop / (row["hip"]["ms_per_image"] * B) / 1e9, 1)
            if twin is not None:
                a, b = enc(px), twin(pixel_values=px)
                ours, theirs = (a.image_embeds, b.image_embeds) if c.projection_dim is not None else (a.last_hidden_state, b.last_hidden_state)
                row["rel_l2_output_vs_transformers_fp16"] = float(f"{float((ours.float() - theirs.float()).norm() / theirs.float().norm()):.3e}")
            r[f"B{B}"] = row
        if twin is None:
            r["transformers"] = "not measured"
        res[name] = r
        del enc, twin
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--no-transformers", action="store_true")
    a = ap.parse_args()
    if a.kernel_stats:
        split = {"kernel_families": dict({"source": "rocprofv3 --kernel-trace --stats over --profile-pass (3 forwards of each tower at B = 16, fp16), folded by "
                                                    "--kernel-stats; shares are of the forwards' own kernels"}, **kernel_split(a.kernel_stats, FAMILIES, SETUP))}
        print(json.dumps(split))
        if a.out:
            update_json(a.out, split)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_vision.py measures on the GPU; none found")
    with torch.no_grad():
        if a.profile_pass:
            from eeg_image_decode_amd import clip_vision
            for name in ("ip_adapter_image_encoder", "git_vision_tower"):
                enc = getattr(clip_vision, name)(dtype=torch.float16, device="cuda")
                px = torch.randn(16, 3, 224, 224, device="cuda", dtype=torch.float16)
                for _ in range(3):
                    enc(px)
                torch.cuda.synchronize()
                del enc
            print(json.dumps({"profile_pass": "3 forwards of each tower at B = 16"}))
            return
        out = {"peak_dense_16bit_TFLOPs": PEAK / 1e12, "timing": "device events around windows of many calls; median of the windows, min / max = spread",
               "attention": attention_rows(a.windows), "towers": tower_rows(a.windows, not a.no_transformers)}
    print(json.dumps(out))
    if a.out:
        update_json(a.out, out)


if __name__ == "__main__":
    main()
