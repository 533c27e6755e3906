"""csrc/self_attn.hip at SDXL's self-attention shapes (16 rows = 8 images x the CFG pair): kernel time and TFLOP/s (4 B heads Tq Tk 64) against
the 2.5 PF/s dense 16-bit MFMA peak, torch's scaled_dot_product_attention on the same tensors as a yardstick, and the SDXL-shaped stand-in
sampling loop's ms per step without / with self-attention.  Prints one JSON object.  Event-bracketed loops of n launches after a warm-up."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eeg_image_decode_amd import sdxl  # noqa: E402

PEAK = 2.5e15
SHAPES = [(16, 4096, 10), (16, 1024, 20)]          # (B, T, heads): the 640-channel and 1280-channel stages at 1024 px


def ev_ms(f, n):
    for _ in range(3):
        f()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    steps = int(os.environ.get("SA_LOOP_STEPS", "10"))
    out = {"peak_dense_16bit_TFLOPs": PEAK / 1e12, "kernel": []}
    with torch.no_grad():
        for dt in (torch.float16, torch.bfloat16):
            for B, T, heads in SHAPES:
                C = heads * 64
                g = torch.Generator(device="cuda").manual_seed(T + heads)
                qkv = torch.randn(B, T, 3 * C, device="cuda", dtype=dt, generator=g)          # fused projection layout, consumed in place
                q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
                o = torch.empty(B, T, C, device="cuda", dtype=dt)
                flop = 4.0 * B * heads * T * T * 64
                n = max(5, int(2e13 / flop * 20))
                ms = ev_ms(lambda: sdxl.self_attention(q, k, v, heads, out=o), n)
                qh, kh, vh = (t.reshape(B, T, heads, 64).transpose(1, 2) for t in (q, k, v))
                ms_ref = ev_ms(lambda: F.scaled_dot_product_attention(qh, kh, vh), n)
                out["kernel"].append({"dtype": str(dt).split(".")[-1], "B": B, "T": T, "heads": heads, "head_dim": 64,
                                      "ms": round(ms, 4), "TFLOPs": round(flop / ms / 1e9, 1), "fraction_of_peak": round(flop / ms / 1e-3 / PEAK, 3),
                                      "torch_sdpa_ms": round(ms_ref, 4), "torch_sdpa_TFLOPs": round(flop / ms_ref / 1e9, 1)})
                del qkv, o
                torch.cuda.empty_cache()
    loop = {}
    for sa in ((False, True) if steps > 0 else ()):                     # SA_LOOP_STEPS=0: kernels only (profiler passes)
        r = sdxl.bench_sampling_loop(images=8, steps=steps, latent=128, self_attention=sa)
        loop["with_self_attention" if sa else "without_self_attention"] = {k: r[k] for k in ("ms_per_step", "attention_stack_TFLOPs", "finite", "workload")}
        torch.cuda.empty_cache()
    out["sampling_loop"] = dict(loop, steps=steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
