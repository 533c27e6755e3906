"""The Inception row's InceptionV3 trunk (eeg_image_decode_amd/metric_nets.InceptionFeatures, csrc/metric_nets.hip) on the GPU at the notebooks' 342 x 342,
fp16.  Prints one JSON object.

  forward       InceptionFeatures.forward for B = 1, 64 and 400 against the same chain from torch's own F.conv2d / F.batch_norm / relu / avg_pool2d / max_pool2d /
                cat on the same weights (NCHW and channels_last), in event-bracketed windows alternated in one process: ms, launches, useful TFLOP/s, ours /
                torch; and the error of `avgpool` against the fp64 restatement over the yardstick's (tests/inception_ref.py) on the benchmark's own images.
  families      (--trace-stats FILE) the kernel families of a `rocprofv3 --kernel-trace --stats` summary of `--trace-run N` (N forwards of one 64-image chunk, in
                a run of its own): time and share per family.

    python tools/bench_inception.py [--out profiles/inception_bench.json] [--windows 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o inception -- python tools/bench_inception.py --trace-run 3
    python tools/bench_inception.py --trace-stats DIR/.../inception_kernel_stats.csv --trace-run 3 [--out profiles/inception_bench.json]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_clip_vision import spread, update_json, window_us  # noqa: E402

SIZE, CHUNK, WARMUP = 342, 64, 2
FAMILIES = (("conv", "convrelu16_kernel"), ("avgpool3x3", "avgpool3x3_16_kernel"), ("maxpool", "maxpool16_kernel"), ("avgpool", "avgpool16_kernel"),
            ("pack", "pack_nchw16_kernel"))          # (the stem's max-pools and the max-pool branches are one kernel)


def useful_flops(net, size=SIZE):
    """2 x multiply-adds of one image's 94 convolutions at their true channel counts (no padding counted)"""
    from eeg_image_decode_amd.metric_nets import INC_STEM, conv_out, pool_out
    h, total = size, 0
    for name, cin, cout, k, s, p in INC_STEM:
        h = conv_out(h, k, s, p)
        total += 2 * h * h * cout * cin * k * k
        if name in ("Conv2d_2b_3x3", "Conv2d_4a_3x3"):
            h = pool_out(h)
    import torch
    for name in net.order:
        blk = getattr(net, name)
        ho = pool_out(h) if blk.kind in "BD" else h
        for m in blk.modules():
            if isinstance(m, torch.nn.Conv2d):
                side = ho if m.stride[0] == 2 else h
                total += 2 * side * side * m.out_channels * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
        h = ho
    return total


def torch_chain(x, sd, net):
    """the trunk from torch's own ops on a torchvision-layout state dict -> (B, 2048) fp32"""
    import torch
    import torch.nn.functional as F
    from eeg_image_decode_amd.metric_nets import INC_FLOW, INC_MEAN, INC_STD, INC_STEM

    def cb(x, key, conv):
        x = F.conv2d(x, sd[f"{key}.conv.weight"], None, stride=conv.stride, padding=conv.padding)
        return F.relu(F.batch_norm(x, sd[f"{key}.bn.running_mean"], sd[f"{key}.bn.running_var"], sd[f"{key}.bn.weight"], sd[f"{key}.bn.bias"], False, 0.0, 1e-3))
    if net.transform_input:
        a = torch.tensor([s / 0.5 for s in INC_STD], device=x.device, dtype=x.dtype)[None, :, None, None]
        b = torch.tensor([(m - 0.5) / 0.5 for m in INC_MEAN], device=x.device, dtype=x.dtype)[None, :, None, None]
        x = x * a + b
    for name, *_ in INC_STEM:
        x = cb(x, name, getattr(net, name).conv)
        if name in ("Conv2d_2b_3x3", "Conv2d_4a_3x3"):
            x = F.max_pool2d(x, 3, 2)
    for name in net.order:
        blk = getattr(net, name)
        t, parts = {"in": x}, []
        for lname, src, dst in INC_FLOW[blk.kind]:
            if lname == "pool":
                y = F.max_pool2d(x, 3, 2) if blk.kind in "BD" else F.avg_pool2d(x, 3, 1, 1)
            else:
                y = cb(t[src], f"{name}.{lname}", getattr(blk, lname).conv)
            if dst == "out":
                parts.append(y)
            else:
                t[dst] = y
        x = torch.cat(parts, 1)
    return F.adaptive_avg_pool2d(x, 1).flatten(1).float()


def forward_rows(net, windows):
    import torch
    sd = {k: (v.to(net.dtype) if v.is_floating_point() else v) for k, v in net.state_dict().items()}       # (torch's batch_norm wants one dtype)
    sd_cl = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd.items()}
    launches = 9 + 8 * net.blocks[0] + 5 + 11 * net.blocks[1] + 7 + 10 * net.blocks[2]
    flops = useful_flops(net)
    rows = {}
    for B in (1, 64, 400):
        x = torch.randn(B, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
        xcl = x.contiguous(memory_format=torch.channels_last)
        fns = {"ours": lambda: net(x), "torch_nchw": lambda: torch_chain(x, sd, net), "torch_channels_last": lambda: torch_chain(xcl, sd_cl, net)}
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        print(f"bench_inception: B = {B} warmed up", file=sys.stderr, flush=True)
        n = 10 if B == 1 else (3 if B == 64 else 1)
        us = {k: [] for k in fns}
        for _ in range(windows):
            for k, f in fns.items():
                us[k].append(window_us(f, n))
        row = {k: dict(spread(v), iterations_per_window=n) for k, v in us.items()}
        ours = row["ours"]["us"]
        row["ours"].update(ms=round(ours / 1e3, 3), launches=launches * ((B + CHUNK - 1) // CHUNK), useful_TFLOP_per_s=round(flops * B / ours / 1e6, 1))
        row["torch_nchw"].update(useful_TFLOP_per_s=round(flops * B / row["torch_nchw"]["us"] / 1e6, 1))
        row["torch_channels_last"].update(useful_TFLOP_per_s=round(flops * B / row["torch_channels_last"]["us"] / 1e6, 1))
        row["ours_over_torch_nchw"] = round(ours / row["torch_nchw"]["us"], 2)
        row["ours_over_torch_channels_last"] = round(ours / row["torch_channels_last"]["us"], 2)
        got, want = net(x), torch_chain(x, sd, net)
        row["rel_l2_vs_torch_fp16"] = float((got - want).norm() / want.norm())
        if B == 1:                                                # the fp64 restatement on the CPU: one image
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import inception_ref as R
            ref, _ = R.features(x, net.state_dict(), net.blocks)
            yard = R.yardstick(x, net.state_dict(), net.blocks, net.dtype)
            e, ey = float((got.cpu().double() - ref).norm() / ref.norm()), float((yard.double() - ref).norm() / ref.norm())
            row["error_vs_fp64"] = {"ours_rel_l2": e, "yardstick_rel_l2": ey, "ratio": round(e / ey, 2)}
        rows[f"B{B}"] = row
    return rows


def trace_run(net, n):
    """WARMUP + n forwards of one chunk: what rocprofv3 traces"""
    import torch
    x = torch.randn(CHUNK, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
    for _ in range(WARMUP + n):
        net(x)
    torch.cuda.synchronize()


def family_rows(path, n):
    """rocprofv3's kernel_stats.csv (Name, Calls, TotalDurationNs, ..) of trace_run(net, n) -> per family: calls, time per forward, share"""
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--trace-stats")
    a = ap.parse_args()
    if a.trace_stats:
        out = {"kernel_trace": family_rows(a.trace_stats, a.trace_run)}
    else:
        import torch
        from eeg_image_decode_amd.metric_nets import inception_v3
        if not torch.cuda.is_available():
            raise SystemExit("bench_inception.py measures on the GPU; none found")
        with torch.no_grad():
            net = inception_v3(dtype=torch.float16, device="cuda", seed=0)
            if a.trace_run:
                return trace_run(net, a.trace_run)
            out = {"job": f"InceptionV3 trunk to avgpool at {SIZE} x {SIZE}, fp16, chunks of {CHUNK} images",
                   "timing": "windows: device events around many calls, ours and torch alternated in one process, median of the windows, min / max = spread",
                   "useful_GFLOP_per_image": round(useful_flops(net) / 1e9, 2),
                   "forward": forward_rows(net, a.windows)}
    print(json.dumps(out))
    if a.out:
        update_json(a.out, out)


if __name__ == "__main__":
    main()
