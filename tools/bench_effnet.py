"""The EffNet-B row's EfficientNet-B1 trunk (eeg_image_decode_amd/metric_nets.EfficientNetFeatures, csrc/metric_nets.hip, csrc/mbconv.hip) on the GPU at the
notebooks' 255 x 255, fp16.  Prints one JSON object.

  forward       EfficientNetFeatures.forward for B = 1, 64 and 400 against the same chain from torch's own F.conv2d(groups=) / F.batch_norm / F.silu / sigmoid /
                adaptive_avg_pool2d on the same weights (NCHW and channels_last), in event-bracketed windows alternated in one process: ms, launches, ours / torch.
  families      (--trace-stats FILE) the kernel families of a `rocprofv3 --kernel-trace --stats` summary of `--trace-run N` (N forwards of one 64-image chunk, in
                a run of its own): time and share per family, and the depthwise family's achieved bytes per second -- the frames it has to read and write once,
                computed from the shapes here -- against the 8 TB/s HBM peak.

    python tools/bench_effnet.py [--out profiles/effnet_bench.json] [--windows 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o effnet -- python tools/bench_effnet.py --trace-run 5
    python tools/bench_effnet.py --trace-stats DIR/.../effnet_kernel_stats.csv --trace-run 5 [--out profiles/effnet_bench.json]
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_clip_vision import spread, update_json, window_us  # noqa: E402

HBM_PEAK = 8.0e12
SIZE, CHUNK, WARMUP = 255, 64, 2
FAMILIES = (("depthwise", "dwconv16_kernel"), ("conv1x1_and_stem", "convrelu16_kernel"), ("gate_multiply", "gate_mul16_kernel"), ("se_gate", "se_gate16_kernel"),
            ("avgpool", "avgpool16_kernel"), ("pack", "pack_nchw16_kernel"))


def depthwise_bytes(net, size=SIZE):
    """bytes one image's depthwise launches must move: each input frame (border included) read once, each output written once, 2 bytes per element of the
    padded channel count, plus the fp32 slabs"""
    from eeg_image_decode_amd.metric_nets import conv_out, pad64
    h, total = conv_out(size, 3, 2, 1), 0
    for _, blk in net.blocks():
        p, c = blk.k // 2, pad64(blk.cexp)
        ho = conv_out(h, blk.k, blk.stride, p)
        slabs = -(-(ho * -(-ho // 4)) // 32)
        total += 2 * c * ((h + 2 * p) ** 2 + ho * ho) + 4 * c * slabs
        h = ho
    return total


def torch_chain(x, sd, layers):
    """the trunk from torch's own ops on a torchvision-layout state dict -> (B, 1280) fp32"""
    import torch
    import torch.nn.functional as F

    def cb(x, key, stride, act=True):
        w = sd[f"{key}.0.weight"]
        x = F.conv2d(x, w, None, stride=stride, padding=w.shape[2] // 2, groups=x.shape[1] // w.shape[1])
        x = F.batch_norm(x, sd[f"{key}.1.running_mean"], sd[f"{key}.1.running_var"], sd[f"{key}.1.weight"], sd[f"{key}.1.bias"], False, 0.0, 1e-5)
        return F.silu(x) if act else x
    from eeg_image_decode_amd.metric_nets import EFF_STAGES
    x = cb(x, "features.0", 2)
    for s, ((expand, _, stride, _, _), n) in enumerate(zip(EFF_STAGES, layers)):
        for i in range(n):
            p, j = f"features.{s + 1}.{i}.block", 0 if expand == 1 else 1
            y = cb(x, f"{p}.0", 1) if expand != 1 else x
            y = cb(y, f"{p}.{j}", stride if i == 0 else 1)
            g = F.adaptive_avg_pool2d(y, 1)
            g = F.silu(F.conv2d(g, sd[f"{p}.{j + 1}.fc1.weight"], sd[f"{p}.{j + 1}.fc1.bias"]))
            y = y * torch.sigmoid(F.conv2d(g, sd[f"{p}.{j + 1}.fc2.weight"], sd[f"{p}.{j + 1}.fc2.bias"]))
            y = cb(y, f"{p}.{j + 2}", 1, act=False)
            x = x + y if i > 0 else y
    return F.adaptive_avg_pool2d(cb(x, "features.8", 1), 1).flatten(1).float()


def forward_rows(net, windows):
    import torch
    sd = {k: (v.to(net.dtype) if v.is_floating_point() else v) for k, v in net.state_dict().items()}       # (torch's batch_norm wants one dtype)
    sd_cl = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd.items()}
    launches = 5 * sum(net.layers) - net.layers[0] + 4
    rows = {}
    for B in (1, 64, 400):
        x = torch.randn(B, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
        xcl = x.contiguous(memory_format=torch.channels_last)
        fns = {"ours": lambda: net(x), "torch_nchw": lambda: torch_chain(x, sd, net.layers), "torch_channels_last": lambda: torch_chain(xcl, sd_cl, net.layers)}
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        print(f"bench_effnet: B = {B} warmed up", file=sys.stderr, flush=True)
        n = 10 if B == 1 else (3 if B == 64 else 1)
        us = {k: [] for k in fns}
        for _ in range(windows):
            for k, f in fns.items():
                us[k].append(window_us(f, n))
        row = {k: dict(spread(v), iterations_per_window=n) for k, v in us.items()}
        ours = row["ours"]["us"]
        row["ours"].update(ms=round(ours / 1e3, 3), launches=launches * ((B + CHUNK - 1) // CHUNK))
        row["ours_over_torch_nchw"] = round(ours / row["torch_nchw"]["us"], 2)
        row["ours_over_torch_channels_last"] = round(ours / row["torch_channels_last"]["us"], 2)
        got, want = net(x), torch_chain(x, sd, net.layers)
        row["rel_l2_vs_torch_fp16"] = float((got - want).norm() / want.norm())
        rows[f"B{B}"] = row
    return rows


def trace_run(net, n):
    """WARMUP + n forwards of one chunk: what rocprofv3 traces"""
    import torch
    x = torch.randn(CHUNK, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
    for _ in range(WARMUP + n):
        net(x)
    torch.cuda.synchronize()


def family_rows(path, net, n):
    """rocprofv3's kernel_stats.csv (Name, Calls, TotalDurationNs, ..) of trace_run(net, n) -> per family: calls, time per forward, share; for the depthwise
    family the achieved bytes per second"""
    fam = {name: {"calls": 0, "ns": 0.0} for name, _ in FAMILIES}
    other = 0.0
    with open(path) as f:
        for r in csv.DictReader(f):
            name, ns, calls = r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])
            hit = next((k for k, pat in FAMILIES if pat in name), None)
            if hit is None:
                other += ns
            else:
                fam[hit]["calls"] += calls
                fam[hit]["ns"] += ns
    forwards = WARMUP + n
    total = sum(v["ns"] for v in fam.values())
    out = {"forwards_traced": forwards, "images_per_forward": CHUNK, "sum_of_kernels_ms_per_forward": round(total / forwards / 1e6, 3),
           "other_kernels_ms_per_forward": round(other / forwards / 1e6, 3), "families": {}}
    for k, v in fam.items():
        out["families"][k] = {"launches_per_forward": v["calls"] / forwards, "ms_per_forward": round(v["ns"] / forwards / 1e6, 4), "share": round(v["ns"] / total, 3) if total else None}
    dw = fam["depthwise"]["ns"] / forwards * 1e-9
    if dw:
        nbytes = depthwise_bytes(net) * CHUNK
        out["families"]["depthwise"].update(bytes_per_forward=nbytes, achieved_TB_per_s=round(nbytes / dw / 1e12, 3), fraction_of_8_TB_per_s=round(nbytes / dw / HBM_PEAK, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--trace-stats")
    a = ap.parse_args()
    import torch
    from eeg_image_decode_amd.metric_nets import efficientnet_b1
    if a.trace_stats:
        out = {"kernel_trace": family_rows(a.trace_stats, efficientnet_b1(dtype=torch.float16, device="cpu", seed=0), a.trace_run)}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_effnet.py measures on the GPU; none found")
        with torch.no_grad():
            net = efficientnet_b1(dtype=torch.float16, device="cuda", seed=0)
            if a.trace_run:
                return trace_run(net, a.trace_run)
            out = {"job": f"EfficientNet-B1 trunk to avgpool at {SIZE} x {SIZE}, fp16, chunks of {CHUNK} images",
                   "timing": "windows: device events around many calls, ours and torch alternated in one process, median of the windows, min / max = spread",
                   "depthwise_bytes_per_image": depthwise_bytes(net),
                   "forward": forward_rows(net, a.windows)}
    print(json.dumps(out))
    if a.out:
        update_json(a.out, out)


if __name__ == "__main__":
    main()
