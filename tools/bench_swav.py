"""The SwAV row's ResNet-50 trunk (eeg_image_decode_amd/metric_nets.ResNetFeatures, csrc/metric_nets.hip) on the GPU at the notebooks' 224 x 224, fp16.
Prints one JSON object.

  stages        every launch of one 64-image chunk by the kernel's own begin .. end (eegclip_time_next_launch), median of `--launches` stamped launches after a
                warm-up, summed per stage (stem, pool, layer1 .. layer4, avgpool) with the stage's useful FLOPs (2 Ho Wo Cout KS^2 Cin per convolution and
                image), its rate and the fraction of the 2.5 PF/s dense 16-bit peak; and the slowest launches by name.
  forward       ResNetFeatures.forward for B = 1, 64 and 400 against the same chain from torch's own F.conv2d / F.batch_norm / relu / max_pool2d / mean on the
                same weights (NCHW and channels_last), in event-bracketed windows alternated in one process: ms, useful TFLOP/s, launches, ours / torch.
  corr_distance metrics.correlation_distance at N = 200, D = 2048 against the torch expression of scipy's definition, the same windows.

    python tools/bench_swav.py [--out profiles/swav_resnet_bench.json] [--windows 5] [--launches 10]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_clip_vision import spread, update_json, window_us  # noqa: E402

PEAK = 2.5e15
SIZE, CHUNK = 224, 64
LAUNCHES = ("eegclip_pack_nchw16_stem", "eegclip_convbn16", "eegclip_maxpool16_pad", "eegclip_avgpool16")


def launch_table(net):
    """[(name, stage, useful FLOPs per image)] of one forward at SIZE, in launch order"""
    from eeg_image_decode_amd.metric_nets import WIDTHS, conv_out, pool_pad_out
    h = conv_out(SIZE, 7, 2, 3)
    rows = [("pack", "pack", 0.0), ("conv1", "stem", 2.0 * h * h * 64 * 49 * 3), ("maxpool", "pool", 0.0)]
    h, cin = pool_pad_out(h), 64
    for s, (width, n) in enumerate(zip(WIDTHS, net.layers)):
        for i in range(n):
            stride = 2 if s > 0 and i == 0 else 1
            ho, st, p = conv_out(h, 3, stride, 1), f"layer{s + 1}", f"layer{s + 1}.{i}"
            rows.append((p + ".conv1", st, 2.0 * h * h * width * cin))
            rows.append((p + ".conv2", st, 2.0 * ho * ho * width * 9 * width))
            if i == 0:
                rows.append((p + ".downsample", st, 2.0 * ho * ho * 4 * width * cin))
            rows.append((p + ".conv3", st, 2.0 * ho * ho * 4 * width * width))
            h, cin = ho, 4 * width
    rows.append(("avgpool", "avgpool", 0.0))
    return rows


def torch_chain(x, sd, layers):
    """the trunk from torch's own ops on a torchvision-layout state dict -> (B, 2048) fp32"""
    import torch.nn.functional as F

    def cb(x, conv, bn, stride, pad, relu=True):
        x = F.conv2d(x, sd[f"{conv}.weight"], None, stride=stride, padding=pad)
        x = F.batch_norm(x, sd[f"{bn}.running_mean"], sd[f"{bn}.running_var"], sd[f"{bn}.weight"], sd[f"{bn}.bias"], False, 0.0, 1e-5)
        return F.relu(x) if relu else x
    x = F.max_pool2d(cb(x, "conv1", "bn1", 2, 3), 3, 2, 1)
    for s, n in enumerate(layers):
        for i in range(n):
            p, stride = f"layer{s + 1}.{i}", 2 if s > 0 and i == 0 else 1
            y = cb(cb(x, p + ".conv1", p + ".bn1", 1, 0), p + ".conv2", p + ".bn2", stride, 1)
            res = cb(x, p + ".downsample.0", p + ".downsample.1", stride, 0, relu=False) if i == 0 else x
            x = F.relu(cb(y, p + ".conv3", p + ".bn3", 1, 0, relu=False) + res)
    return x.float().mean((2, 3))


class ArmAt:
    """the loaded library with the stamp events armed in front of the k-th kernel launch made through it (metric_nets fetches the library per call)"""

    def __init__(self, L, k, e0, e1):
        self.L, self.k, self.e0, self.e1, self.n = L, k, e0, e1, 0

    def __getattr__(self, name):
        fn = getattr(self.L, name)
        if name not in LAUNCHES:
            return fn

        def call(*a):
            if self.n == self.k:
                self.L.eegclip_time_next_launch(self.e0, self.e1)
            self.n += 1
            return fn(*a)
        return call


def stage_rows(net, launches):
    import torch
    import eeg_image_decode_amd.metric_nets as MN
    from eeg_image_decode_amd._lib import lib
    L = lib()
    e0, e1 = L.eegclip_timing_event_create(), L.eegclip_timing_event_create()
    x = torch.randn(CHUNK, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
    table = launch_table(net)
    for _ in range(3):
        net(x)
    torch.cuda.synchronize()
    us, keep = [], MN.lib
    try:
        for k in range(len(table)):
            got = []
            for _ in range(launches):
                proxy = ArmAt(L, k, e0, e1)
                MN.lib = lambda: proxy
                net(x)
                torch.cuda.synchronize()
                assert proxy.n == len(table)
                got.append(float(L.eegclip_timing_elapsed_ms(e0, e1)) * 1e3)
            us.append(got)
    finally:
        MN.lib = keep
    L.eegclip_timing_event_destroy(e0)
    L.eegclip_timing_event_destroy(e1)
    med = [statistics.median(g) for g in us]
    stages = {}
    for (name, stage, fl), m, g in zip(table, med, us):
        r = stages.setdefault(stage, {"launches": 0, "kernel_us": 0.0, "min_us": 0.0, "max_us": 0.0, "useful_GFLOP_per_image": 0.0})
        r["launches"] += 1
        r["kernel_us"] += m
        r["min_us"] += min(g)
        r["max_us"] += max(g)
        r["useful_GFLOP_per_image"] += fl / 1e9
    for r in stages.values():
        f = r["useful_GFLOP_per_image"] * 1e9 * CHUNK
        if f:
            r.update(useful_TFLOPs=round(f / r["kernel_us"] / 1e6, 1), fraction_of_peak=round(f / (r["kernel_us"] * 1e-6) / PEAK, 4))
        for k in ("kernel_us", "min_us", "max_us"):
            r[k] = round(r[k], 2)
        r["useful_GFLOP_per_image"] = round(r["useful_GFLOP_per_image"], 4)
    slow = sorted(zip(med, table), reverse=True)[:8]
    slowest = [{"launch": t[0], "kernel_us": round(m, 2), "useful_TFLOPs": round(t[2] * CHUNK / m / 1e6, 1)} for m, t in slow]
    return {"stamped_launches_each": launches, "sum_of_kernels_us": round(sum(med), 2), "stages": stages, "slowest_launches": slowest}


def forward_rows(net, windows):
    import torch
    sd = net.state_dict()
    sd_cl = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd.items()}
    table = launch_table(net)
    total = sum(t[2] for t in table)
    rows = {}
    for B in (1, 64, 400):
        x = torch.randn(B, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
        xcl = x.contiguous(memory_format=torch.channels_last)
        fns = {"ours": lambda: net(x), "torch_nchw": lambda: torch_chain(x, sd, net.layers), "torch_channels_last": lambda: torch_chain(xcl, sd_cl, net.layers)}
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        n = 10 if B == 1 else (3 if B == 64 else 1)
        us = {k: [] for k in fns}
        for _ in range(windows):
            for k, f in fns.items():
                us[k].append(window_us(f, n))
        row = {k: dict(spread(v), iterations_per_window=n) for k, v in us.items()}
        ours = row["ours"]["us"]
        row["ours"].update(ms=round(ours / 1e3, 3), launches=len(table) * ((B + CHUNK - 1) // CHUNK), useful_TFLOPs_end_to_end=round(total * B / ours / 1e6, 1),
                           fraction_of_peak_end_to_end=round(total * B / (ours * 1e-6) / PEAK, 4))
        row["ours_over_torch_nchw"] = round(ours / row["torch_nchw"]["us"], 2)
        row["ours_over_torch_channels_last"] = round(ours / row["torch_channels_last"]["us"], 2)
        got, want = net(x), torch_chain(x, sd, net.layers)
        row["rel_l2_vs_torch_fp16"] = float((got - want).norm() / want.norm())
        rows[f"B{B}"] = row
    return rows


def corr_rows(windows):
    import torch
    from eeg_image_decode_amd import metrics
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randn(200, 2048, device="cuda", generator=g).abs()
    b = 0.6 * a + 0.8 * torch.randn(200, 2048, device="cuda", generator=g).abs()

    def ref():
        x, y = a - a.mean(1, keepdim=True), b - b.mean(1, keepdim=True)
        return 1 - (x * y).sum(1) / (x.norm(dim=1) * y.norm(dim=1))
    fns = {"ours": lambda: metrics.correlation_distance(a, b), "torch": ref}
    for f in fns.values():
        for _ in range(3):
            f()
    us = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            us[k].append(window_us(f, 50))
    row = {k: dict(spread(v), iterations_per_window=50) for k, v in us.items()}
    row["ours_over_torch"] = round(row["ours"]["us"] / row["torch"]["us"], 2)
    row["max_abs_diff_vs_torch_fp64"] = float((fns["ours"]().double() - (1 - torch.stack([torch.corrcoef(torch.stack([a[i].double(), b[i].double()]))[0, 1]
                                                                                         for i in range(200)]))).abs().max())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_swav.py measures on the GPU; none found")
    from eeg_image_decode_amd.metric_nets import swav_resnet50
    with torch.no_grad():
        net = swav_resnet50(dtype=torch.float16, device="cuda", seed=0)
        total = sum(t[2] for t in launch_table(net))
        out = {"job": f"ResNet-50 trunk to avgpool at {SIZE} x {SIZE}, fp16, chunks of {CHUNK} images",
               "peak_dense_16bit_TFLOPs": PEAK / 1e12,
               "useful_GFLOP_per_image": round(total / 1e9, 3),
               "timing": "kernel_us: the launch's own begin / end timestamps, median of stamped launches; windows: device events around many calls, ours and torch "
                         "alternated in one process, median of the windows, min / max = spread",
               "chunk_of_64": stage_rows(net, a.launches),
               "forward": forward_rows(net, a.windows),
               "corr_distance_N200_D2048": corr_rows(a.windows)}
    print(json.dumps(out))
    if a.out:
        update_json(a.out, out)


if __name__ == "__main__":
    main()
