"""ms per SDXLUNet forward (SDXL config + IP-Adapter, fp16) at 512 x 512 with B = 1 (sdxl-turbo) and at 1024 x 1024 with B = 2 (a classifier-free-guidance
pair), after warm-up, over --reps repetitions (median and min of per-forward CUDA-event times); algorithmic FLOPs from the layer shapes
(sdxl_unet.forward_flops) and their share of the dense 16-bit peak.  Writes profiles/sdxl_unet_bench.json (--out).

    python tools/bench_sdxl_unet.py [--reps 10] [--out profiles/sdxl_unet_bench.json] [--only 512|1024]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from eeg_image_decode_amd.sdxl_unet import SDXLUNet, forward_flops  # noqa: E402

PEAK_16BIT_TFLOPS = 2500.0          # MI355X dense fp16 / bf16 matrix peak, approximately (spec sheet figure)


def bench(unet, B, L, reps, warmup=2):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 4, L, L, generator=g).to("cuda", unet.dtype)
    ehs = (torch.randn(B, 77, 2048, generator=g) * 0.5).to("cuda", unet.dtype)
    added = {"text_embeds": (torch.randn(B, 1280, generator=g) * 0.5).to("cuda", unet.dtype),
             "time_ids": torch.tensor([[8 * L, 8 * L, 0, 0, 8 * L, 8 * L]] * B, dtype=unet.dtype, device="cuda"),
             "image_embeds": torch.randn(B, 1024, generator=g).to("cuda", unet.dtype)}
    unet.precompute(ehs, added["image_embeds"])
    for _ in range(warmup):
        y = unet(x, 999, encoder_hidden_states=ehs, added_cond_kwargs=added)[0]
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = unet(x, 999, encoder_hidden_states=ehs, added_cond_kwargs=added)[0]
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    fl = forward_flops(unet, B, L, L)
    total = sum(fl.values())
    med = statistics.median(ms)
    return {"pixels": f"{8 * L}x{8 * L}", "batch": B, "dtype": str(unet.dtype).split(".")[-1], "reps": reps, "ms_median": round(med, 3),
            "ms_min": round(min(ms), 3), "GFLOP_per_image": round(total / B / 1e9, 1),
            "flop_share": {k: round(v / total, 3) for k, v in fl.items()},
            "TFLOPs_at_median": round(total / med / 1e9, 1), "fraction_of_16bit_peak": round(total / med / 1e9 / PEAK_16BIT_TFLOPS, 3),
            "finite": bool(torch.isfinite(y.float()).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdxl_unet_bench.json"))
    ap.add_argument("--only", choices=["512", "1024"])
    a = ap.parse_args()
    unet = SDXLUNet(dtype=torch.float16, device="cuda", ip_adapter=True)
    rows = []
    if a.only in (None, "512"):
        rows.append(bench(unet, 1, 64, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if a.only in (None, "1024"):
        rows.append(bench(unet, 2, 128, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    res = {"what": "SDXLUNet forward (SDXL config + IP-Adapter, random default-init weights), HIP kernels only", "device": torch.cuda.get_device_name(0),
           "peak_16bit_TFLOPs_assumed": PEAK_16BIT_TFLOPS, "runs": rows}
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
