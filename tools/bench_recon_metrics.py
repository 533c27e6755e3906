"""Reconstruction metrics (eeg_image_decode_amd/metrics.py, csrc/recon_metrics.hip) on the GPU.  Prints one JSON object.

  pixcorr_ssim  eegclip_pixcorr_ssim on 200 pairs of 425 x 425 (the reference's 200 test images after Resize(425)), fp32 and fp16 planes: the tile kernel's own
                begin .. end (eegclip_time_next_launch: the timestamps of the launch itself; the finalize launch behind it adds 200 x 189 rows of 80 bytes) as
                the median of `--launches` stamped launches after a warm-up; beside it the time the input bytes take at 8 TB/s and the ratio of the two; the
                whole call (both launches + the workspace allocation) in event-bracketed windows; and the largest error of the first 4 pairs against scipy in fp64.
  torch         the same metrics composed from torch ops on the same GPU and the same tensors: gray by a weighted sum, the five fields through F.conv2d with
                the 11 x 11 Gaussian, S and its cropped mean; torch.corrcoef per pair.  In the same windows, alternating with ours.
  scipy         the fp64 definition (scipy.ndimage.gaussian_filter, np.corrcoef) on one CPU core, per pair.
  two_way       eegclip_two_way at N = 200 with D = 768 and D = 46656: the call (stats + tile + counts launches) in windows, the stats kernel stamped, the time
                the 2 N D 4 input bytes take at 8 TB/s; torch.corrcoef of the stacked (400, D) matrix + the comparison, in the same windows; np.corrcoef
                on one core.

    python tools/bench_recon_metrics.py [--out profiles/recon_metrics_bench.json] [--windows 7] [--launches 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_clip_vision import spread, update_json, window_us  # noqa: E402

HBM = 8e12
PAIRS, SIZE, N = 200, 425, 200


def taps():
    import numpy as np
    i = np.arange(-5, 6, dtype=np.float64)
    w = np.exp(-i * i / 4.5)
    return w / w.sum()


def scipy_pair(a, b):
    """(3, H, W) float arrays -> (pixcorr, ssim) in fp64"""
    import numpy as np
    from scipy.ndimage import gaussian_filter
    a, b = a.astype(np.float64), b.astype(np.float64)
    x, y = 0.2125 * a[0] + 0.7154 * a[1] + 0.0721 * a[2], 0.2125 * b[0] + 0.7154 * b[1] + 0.0721 * b[2]
    f = lambda z: gaussian_filter(z, 1.5, truncate=3.5)
    ux, uy = f(x), f(y)
    vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
    S = (2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    return float(np.corrcoef(a.ravel(), b.ravel())[0, 1]), float(S[5:-5, 5:-5].mean())


def one_core():
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    except (AttributeError, OSError):
        pass


def image_rows(windows, launches):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from eeg_image_decode_amd import metrics as M
    from eeg_image_decode_amd._lib import lib
    L = lib()
    e0, e1 = L.eegclip_timing_event_create(), L.eegclip_timing_event_create()
    g = torch.Generator(device="cuda").manual_seed(1)
    base = F.interpolate(torch.rand(PAIRS, 3, 20, 20, device="cuda", generator=g), size=(SIZE, SIZE), mode="bilinear")     # smooth images
    a32 = base.clamp(0, 1).contiguous()
    b32 = (base + 0.1 * torch.randn(PAIRS, 3, SIZE, SIZE, device="cuda", generator=g)).clamp(0, 1).contiguous()
    w2 = torch.from_numpy(np.outer(taps(), taps())).float().cuda().reshape(1, 1, 11, 11).repeat(5, 1, 1, 1)
    gw = torch.tensor([0.2125, 0.7154, 0.0721], device="cuda").reshape(1, 3, 1, 1)

    def torch_metrics(a, b):
        a, b = a.float(), b.float()
        x, y = (a * gw).sum(1, keepdim=True), (b * gw).sum(1, keepdim=True)
        m = F.conv2d(torch.cat([x, y, x * x, y * y, x * y], 1), w2, groups=5)
        ux, uy = m[:, 0], m[:, 1]
        vx, vy, vxy = m[:, 2] - ux * ux, m[:, 3] - uy * uy, m[:, 4] - ux * uy
        S = (2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
        pc = torch.stack([torch.corrcoef(torch.stack([a[i].reshape(-1), b[i].reshape(-1)]))[0, 1] for i in range(a.shape[0])])
        return pc, S.mean((1, 2))

    rows = {}
    for name, a, b in (("fp32", a32, b32), ("fp16", a32.half(), b32.half())):
        ours, theirs = (lambda: M.pixcorr_ssim(a, b, size=None)), (lambda: torch_metrics(a, b))
        for f in (ours, theirs):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        stamped = []
        for _ in range(launches):
            L.eegclip_time_next_launch(e0, e1)
            ours()
            torch.cuda.synchronize()
            stamped.append(float(L.eegclip_timing_elapsed_ms(e0, e1)) * 1e3)
        us = {"ours": [], "torch": []}
        for _ in range(windows):
            us["ours"].append(window_us(ours, 20))
            us["torch"].append(window_us(theirs, 3))
        pix, ssm = ours()
        tp, ts = theirs()
        want = [scipy_pair(a[i].float().cpu().numpy(), b[i].float().cpu().numpy()) for i in range(4)]
        nbytes = 2 * a.numel() * a.element_size()
        k_us, floor_us = statistics.median(stamped), nbytes / HBM * 1e6
        rows[name] = {"kernel_us": round(k_us, 2), "kernel_min_us": round(min(stamped), 2), "kernel_max_us": round(max(stamped), 2), "stamped_launches": launches,
                      "input_bytes": nbytes, "us_at_8TBps": round(floor_us, 2), "kernel_over_bytes_at_8TBps": round(k_us / floor_us, 2),
                      "call_in_windows": dict(spread(us["ours"]), iterations_per_window=20),
                      "torch_conv2d_corrcoef": dict(spread(us["torch"]), iterations_per_window=3),
                      "torch_over_ours_window": round(statistics.median(us["torch"]) / statistics.median(us["ours"]), 1),
                      "max_abs_error_vs_scipy_fp64_4_pairs": {"ssim": float(max(abs(float(ssm[i]) - want[i][1]) for i in range(4))),
                                                              "pixcorr": float(max(abs(float(pix[i]) - want[i][0]) for i in range(4))),
                                                              "torch_ssim": float(max(abs(float(ts[i]) - want[i][1]) for i in range(4))),
                                                              "torch_pixcorr": float(max(abs(float(tp[i]) - want[i][0]) for i in range(4)))},
                      "ssim_mean": round(float(ssm.mean()), 4), "pixcorr_mean": round(float(pix.mean()), 4)}
    L.eegclip_timing_event_destroy(e0)
    L.eegclip_timing_event_destroy(e1)
    pair = (a32[0].cpu().numpy(), b32[0].cpu().numpy())
    return rows, pair


def two_way_rows(windows, launches):
    import numpy as np
    import torch
    from eeg_image_decode_amd import metrics as M
    from eeg_image_decode_amd._lib import lib
    L = lib()
    e0, e1 = L.eegclip_timing_event_create(), L.eegclip_timing_event_create()
    rows = {}
    for D in (768, 46656):
        g = torch.Generator(device="cuda").manual_seed(D)
        G = torch.randn(N, D, device="cuda", generator=g)
        P = 0.35 * G + torch.randn(N, D, device="cuda", generator=g)

        def theirs():
            r = torch.corrcoef(torch.cat([G, P]))[:N, N:]
            return (r < r.diagonal()[None, :]).sum(0).float().mean() / (N - 1)

        ours = lambda: M.two_way_identification(G, P, return_counts=True)[1]
        for f in (ours, theirs):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        stamped = []
        for _ in range(launches):
            L.eegclip_time_next_launch(e0, e1)
            ours()
            torch.cuda.synchronize()
            stamped.append(float(L.eegclip_timing_elapsed_ms(e0, e1)) * 1e3)
        us = {"ours": [], "torch": []}
        for _ in range(windows):
            us["ours"].append(window_us(ours, 20))
            us["torch"].append(window_us(theirs, 20))
        one_core()
        g64, p64 = G.double().cpu().numpy(), P.double().cpu().numpy()
        t0 = time.perf_counter()
        r = np.corrcoef(g64, p64)[:N, N:]
        want = ((r < np.diag(r)[None, :]) & ~np.eye(N, dtype=bool)).sum(0)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        nbytes = 2 * N * D * 4
        floor_us = nbytes / HBM * 1e6
        rows[f"D{D}"] = {"N": N, "D": D, "call_in_windows": dict(spread(us["ours"]), iterations_per_window=20, note="three launches + float(count.sum()) on the host"),
                         "stats_kernel_us": round(statistics.median(stamped), 2), "input_bytes": nbytes, "us_at_8TBps": round(floor_us, 2),
                         "call_over_bytes_at_8TBps": round(statistics.median(us["ours"]) / floor_us, 1),
                         "torch_corrcoef": dict(spread(us["torch"]), iterations_per_window=20),
                         "torch_over_ours_window": round(statistics.median(us["torch"]) / statistics.median(us["ours"]), 2),
                         "numpy_corrcoef_one_core_ms": round(cpu_ms, 2), "counts_equal_numpy_fp64": bool(np.array_equal(ours().cpu().numpy(), want))}
    L.eegclip_timing_event_destroy(e0)
    L.eegclip_timing_event_destroy(e1)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon_metrics.py measures on the GPU; none found")
    with torch.no_grad():
        images, pair = image_rows(a.windows, a.launches)
        out = {"job": f"{PAIRS} pairs of {SIZE} x {SIZE} (3 planes each); two-way at N = {N}",
               "timing": "kernel_us: the launch's own begin / end timestamps, median of stamped launches; windows: device events around many calls, median of the "
                         "windows, min / max = spread",
               "pixcorr_ssim": images, "two_way": two_way_rows(a.windows, a.launches)}
    one_core()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        scipy_pair(*pair)
        t.append((time.perf_counter() - t0) * 1e3)
    out["scipy_one_core"] = {"ms_per_pair": round(statistics.median(t), 2), "min_ms": round(min(t), 2), "max_ms": round(max(t), 2), "repeats": 3,
                             "ms_for_200_pairs": round(statistics.median(t) * PAIRS, 1)}
    print(json.dumps(out))
    if a.out:
        update_json(a.out, out)


if __name__ == "__main__":
    main()
