"""AlexNet features (eeg_image_decode_amd/metric_nets.py, csrc/metric_nets.hip) on the GPU at the notebooks' 256 x 256, fp16.  Prints one JSON object.

  layers    every launch of one 64-image chunk by the kernel's own begin .. end (eegclip_time_next_launch), median of `--launches` stamped launches after a
            warm-up; for the convolutions the useful FLOPs (2 Ho Wo Cout KS^2 Cin per image: 184.4 + 590.4 + 298.6 + 398.1 + 265.4 MFLOP), the rate and the
            fraction of the 2.5 PF/s dense 16-bit peak; beside each the same layer through torch (F.conv2d + relu, F.max_pool2d; NCHW and channels_last) in
            event-bracketed windows alternated with ours.
  forward   AlexNetFeatures.forward (both nodes; 8 launches per 64-image chunk) for B = 1, 64 and 400 against torch's own chain of the same layers on the
            same weights, in the same windows, alternating; ms, useful TFLOP/s of the whole call, and ours / torch.
  accuracy  relative L2 of both nodes to an fp64 restatement on the CPU over the same figure for the 16-bit yardstick (the chain in fp32 with the input, the
            weights and every layer's output rounded to the dtype), at 67 x 83 (N = 8) and 256 x 256 (N = 2), fp16 and bf16, on this tool's own smooth
            images and its own restatement of the chain (the tests measure the same ratio on their images with tests/metric_nets_ref.py).

    python tools/bench_metric_nets.py [--out profiles/metric_nets_bench.json] [--windows 5] [--launches 20]
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
SIZE, CHUNK = 256, 64
ORDER = ("0", "3", "6", "8", "10")


def torch_chain(x, sd):
    """torchvision AlexNet's layers up to features.11 from torch's own ops -> (features.4, features.11)"""
    import torch.nn.functional as F
    from eeg_image_decode_amd.metric_nets import CONVS
    f4 = None
    for i in ORDER:
        _, _, _, s, p = CONVS[i]
        x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"], sd[f"features.{i}.bias"], stride=s, padding=p))
        if i == "3":
            f4 = x
        if i in ("0", "3"):
            x = F.max_pool2d(x, 3, 2)
    return f4, x


def flops_per_image():
    from eeg_image_decode_amd.metric_nets import CONVS, conv_out, pool_out
    out, n = {}, SIZE
    for i in ORDER:
        cin, cout, k, s, p = CONVS[i]
        n = conv_out(n, k, s, p)
        out[i] = 2.0 * n * n * cout * k * k * cin
        if i in ("0", "3"):
            n = pool_out(n)
    return out


class ArmAt:
    """the loaded library with the stamp events armed in front of the k-th kernel launch made through it (metric_nets fetches the library per call)"""
    LAUNCHES = ("eegclip_pack_nchw16", "eegclip_convrelu16", "eegclip_maxpool16")

    def __init__(self, L, k, e0, e1):
        self.L, self.k, self.e0, self.e1, self.n = L, k, e0, e1, 0

    def __getattr__(self, name):
        fn = getattr(self.L, name)
        if name not in self.LAUNCHES:
            return fn

        def call(*a):
            if self.n == self.k:
                self.L.eegclip_time_next_launch(self.e0, self.e1)
            self.n += 1
            return fn(*a)
        return call


def layer_rows(net, windows, launches):
    """the 8 launches of one chunk, each stamped; torch's op for the same layer in windows"""
    import torch
    import torch.nn.functional as F
    import eeg_image_decode_amd.metric_nets as MN
    from eeg_image_decode_amd._lib import lib
    from eeg_image_decode_amd.metric_nets import CONVS
    L = lib()
    e0, e1 = L.eegclip_timing_event_create(), L.eegclip_timing_event_create()
    x = torch.randn(CHUNK, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
    names = ["pack", "features.0", "pool.2", "features.3", "pool.5", "features.6", "features.8", "features.10"]
    for _ in range(3):
        net(x)
    torch.cuda.synchronize()
    stamped = {n: [] for n in names}
    keep = MN.lib
    try:
        for k, name in enumerate(names):
            for _ in range(launches):
                proxy = ArmAt(L, k, e0, e1)
                MN.lib = lambda: proxy
                net(x)
                torch.cuda.synchronize()
                stamped[name].append(float(L.eegclip_timing_elapsed_ms(e0, e1)) * 1e3)
    finally:
        MN.lib = keep
    L.eegclip_timing_event_destroy(e0)
    L.eegclip_timing_event_destroy(e1)
    # torch's op per layer, on the activations of its own chain
    sd = net.state_dict()
    acts, t = {}, x
    for i in ORDER:
        _, _, _, s, p = CONVS[i]
        acts[f"features.{i}"] = t
        t = F.relu(F.conv2d(t, sd[f"features.{i}.weight"], sd[f"features.{i}.bias"], stride=s, padding=p))
        if i in ("0", "3"):
            acts["pool.2" if i == "0" else "pool.5"] = t
            t = F.max_pool2d(t, 3, 2)
    fl = flops_per_image()
    rows = {}
    for name in names:
        us = statistics.median(stamped[name])
        row = {"kernel_us": round(us, 2), "min_us": round(min(stamped[name]), 2), "max_us": round(max(stamped[name]), 2), "stamped_launches": launches}
        if name.startswith("features."):
            i = name.split(".")[1]
            _, _, _, s, p = CONVS[i]
            f = fl[i] * CHUNK
            row.update(useful_MFLOP_per_image=round(fl[i] / 1e6, 1), useful_TFLOPs=round(f / us / 1e6, 1), fraction_of_peak=round(f / (us * 1e-6) / PEAK, 4))
            w, b = sd[f"{name}.weight"], sd[f"{name}.bias"]
            for fmt in ("nchw", "channels_last"):
                a = acts[name] if fmt == "nchw" else acts[name].contiguous(memory_format=torch.channels_last)
                wt = w if fmt == "nchw" else w.contiguous(memory_format=torch.channels_last)
                op = lambda a=a, wt=wt: F.relu(F.conv2d(a, wt, b, stride=s, padding=p))
                for _ in range(3):
                    op()
                row[f"torch_{fmt}"] = spread([window_us(op, 10) for _ in range(windows)])
        elif name.startswith("pool."):
            op = lambda a=acts[name]: F.max_pool2d(a, 3, 2)
            for _ in range(3):
                op()
            row["torch_nchw"] = spread([window_us(op, 10) for _ in range(windows)])
        rows[name] = row
    return rows


def forward_rows(net, windows):
    import torch
    sd = net.state_dict()
    sd_cl = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd.items()}
    total = sum(flops_per_image().values())
    rows = {}
    for B in (1, 64, 400):
        x = torch.randn(B, 3, SIZE, SIZE, device="cuda", dtype=net.dtype)
        xcl = x.contiguous(memory_format=torch.channels_last)
        fns = {"ours": lambda: net(x), "torch_nchw": lambda: torch_chain(x, sd), "torch_channels_last": lambda: torch_chain(xcl, sd_cl)}
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        n = 20 if B == 1 else (5 if B == 64 else 2)
        us = {k: [] for k in fns}
        for _ in range(windows):
            for k, f in fns.items():
                us[k].append(window_us(f, n))
        row = {k: dict(spread(v), iterations_per_window=n) for k, v in us.items()}
        ours = row["ours"]["us"]
        row["ours"].update(ms=round(ours / 1e3, 3), useful_TFLOPs_end_to_end=round(total * B / ours / 1e6, 1), fraction_of_peak_end_to_end=round(total * B / (ours * 1e-6) / PEAK, 4))
        best = min(row["torch_nchw"]["us"], row["torch_channels_last"]["us"])
        row["ours_over_torch_nchw"] = round(ours / row["torch_nchw"]["us"], 2)
        row["ours_over_best_torch"] = round(ours / best, 2)
        got, want = net(x), torch_chain(x, sd)
        row["max_abs_diff_vs_torch_fp16"] = {"features.4": float((got["features.4"].float() - want[0].float()).abs().max()),
                                             "features.11": float((got["features.11"].float() - want[1].float()).abs().max())}
        rows[f"B{B}"] = row
    return rows


def accuracy_rows():
    """product error / yardstick error against an fp64 restatement on the CPU, seeded weights, this tool's own smooth images (sinusoids, one phase set per image)"""
    import numpy as np
    import torch
    from eeg_image_decode_amd.metric_nets import AlexNetFeatures
    rows = {}
    for H, W, N in ((67, 83, 8), (SIZE, SIZE, 2)):
        yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
        rng = np.random.default_rng(0)
        ph = rng.uniform(0, 2 * np.pi, (N, 3, 2))
        img = np.stack([np.stack([0.5 + 0.35 * np.sin(5 * xx + ph[n, c, 0]) * np.cos(4 * yy + ph[n, c, 1]) for c in range(3)]) for n in range(N)])
        x32 = (torch.from_numpy(img).float() - torch.tensor([0.485, 0.456, 0.406])[None, :, None, None]) / torch.tensor([0.229, 0.224, 0.225])[None, :, None, None]
        for dt in (torch.float16, torch.bfloat16):
            net = AlexNetFeatures(dtype=dt, device="cuda", seed=0)
            x = x32.to(dt)
            got = net(x.cuda())
            sd = {k: v.cpu() for k, v in net.state_dict().items()}
            ref = torch_chain(x.double(), {k: v.double() for k, v in sd.items()})
            rnd = lambda t: t.to(dt).float()
            yard, t = [], rnd(x.float())
            from eeg_image_decode_amd.metric_nets import CONVS
            import torch.nn.functional as F
            for i in ORDER:
                _, _, _, s, p = CONVS[i]
                t = rnd(F.relu(F.conv2d(t, sd[f"features.{i}.weight"].float(), sd[f"features.{i}.bias"].float(), stride=s, padding=p)))
                if i in ("3", "10"):
                    yard.append(t)
                if i in ("0", "3"):
                    t = F.max_pool2d(t, 3, 2)
            row = {}
            for k, node in enumerate(("features.4", "features.11")):
                e = float((got[node].cpu().double() - ref[k]).norm() / ref[k].norm())
                ey = float((yard[k].double() - ref[k]).norm() / ref[k].norm())
                row[node] = {"rel_l2": float(f"{e:.3e}"), "yardstick_rel_l2": float(f"{ey:.3e}"), "ratio": round(e / ey, 3)}
            rows[f"{H}x{W}_N{N}_{'fp16' if dt == torch.float16 else 'bf16'}"] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_metric_nets.py measures on the GPU; none found")
    from eeg_image_decode_amd.metric_nets import AlexNetFeatures
    with torch.no_grad():
        net = AlexNetFeatures(dtype=torch.float16, device="cuda", seed=0)
        fl = flops_per_image()
        out = {"job": f"AlexNet features.4 / features.11 at {SIZE} x {SIZE}, fp16, chunks of {CHUNK} images",
               "peak_dense_16bit_TFLOPs": PEAK / 1e12,
               "useful_GFLOP_per_image": round(sum(fl.values()) / 1e9, 3),
               "timing": "kernel_us: the launch's own begin / end timestamps, median of stamped launches; windows: device events around many calls, ours and torch "
                         "alternated in one process, median of the windows, min / max = spread",
               "layers_chunk_of_64": layer_rows(net, a.windows, a.launches),
               "forward": forward_rows(net, a.windows),
               "accuracy_vs_fp64": accuracy_rows()}
    print(json.dumps(out))
    if a.out:
        update_json(a.out, out)


if __name__ == "__main__":
    main()
